"""The randomised edit driver (tests/edit_sequence.py) on its reference side alone: the CPU oracle, the restatements of the edit
calls and the oracle's set_scene_state hook, over the driver's default seeds (edit_sequence.DEFAULT_SEEDS).  The oracle's structure is
checked after every call, and the seeds together must reach every corner the driver counts — so that the GPU test, which runs the
same seeds, cannot pass by never getting there."""
import pytest

from tests import edit_sequence as es


@pytest.fixture(scope="module")
def runs():
    return {seed: es.run_sequence(seed, structure=True) for seed in es.DEFAULT_SEEDS}


def test_every_kind_of_settings_occurs(runs):
    assert {r["kind"] for r in runs.values()} == set(es.KINDS)


@pytest.mark.parametrize("counter", es.COUNTERS)
def test_the_default_seeds_reach_every_corner(runs, counter):
    per_seed = {seed: r["counters"][counter] for seed, r in runs.items()}
    assert sum(per_seed.values()) >= 1, per_seed


def test_structure_is_checked_after_every_call(runs):
    """check_structure ran after every call of every seed; its block accounting is exact except behind a frame that ran out of excess
    entries (which gives up blocks, as upstream does) — and only a seed with a cut excess list (kind b) can get there"""
    for seed, r in runs.items():
        exact, given_up = r["structure_checks"]
        assert exact + given_up == len(r["log"]), (seed, r["structure_checks"], len(r["log"]))
        assert given_up == 0 or r["kind"] == "b", (seed, r["kind"], r["structure_checks"])


def test_sequences_are_reproducible_and_hold_edits_and_readers(runs):
    again = es.run_sequence(es.DEFAULT_SEEDS[0])
    assert again["log"] == runs[es.DEFAULT_SEEDS[0]]["log"] and again["counters"] == runs[es.DEFAULT_SEEDS[0]]["counters"]
    kinds = {call[0] for r in runs.values() for call in r["log"]}
    assert kinds >= {"frame", "decay", "render", "reset", "erase", "crop", "erase_volume", "merge", "import", "snapshot", "reader"}, kinds
    assert {call[1] for r in runs.values() for call in r["log"] if call[0] == "reader"} == set(es.READERS)
