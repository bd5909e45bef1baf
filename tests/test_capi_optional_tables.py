"""The optional tables of dynslam_amd/_capi.py (every header next to include/dsr.h): ONE binder and ONE registry bind them, the
binders of old are names for its entries, and ONE cache on the backend's api object keeps what was bound — a slot per table's name.
Against the built libdsr_hip.so; no compute calls (runs without a GPU)."""
import ctypes as C
import os
from types import SimpleNamespace

import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, optional_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("track", "gc", "eval", "snapshot", "mesh", "merge", "align", "dense", "esdf", "query", "heightmap", "erase", "components")
# (key, the version function the stub answers wrongly, the ImportError's text)
MISMATCHES = [("track", "track_abi_version", "tracker ABI version mismatch (include/dsr_track.h)"),
              ("gc", "gc_abi_version", "batch GC ABI version mismatch (include/dsr_gc.h)"),
              ("eval", "eval_abi_version", "evaluator ABI version mismatch (include/dsr_eval.h)"),
              ("snapshot", "snapshot_abi_version", "snapshot ABI version mismatch (include/dsr_snapshot.h)"),
              ("mesh", "mesh_abi_version", "complete mesher ABI version mismatch (include/dsr_mesh.h)"),
              ("mesh", "mesh_indexed_abi_version", "indexed mesher ABI version mismatch (include/dsr_mesh.h)"),
              ("merge", "merge_abi_version", "merge ABI version mismatch (include/dsr_merge.h)"),
              ("align", "align_abi_version", "align ABI version mismatch (include/dsr_align.h)"),
              ("dense", "dense_abi_version", "dense ABI version mismatch (include/dsr_dense.h)"),
              ("esdf", "esdf_abi_version", "esdf ABI version mismatch (include/dsr_esdf.h)"),
              ("query", "query_abi_version", "query ABI version mismatch (include/dsr_query.h)"),
              ("heightmap", "heightmap_abi_version", "heightmap ABI version mismatch (include/dsr_heightmap.h)"),
              ("erase", "erase_abi_version", "erase ABI version mismatch (include/dsr_erase.h)"),
              ("components", "components_abi_version", "components ABI version mismatch (include/dsr_components.h)")]


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    return C.CDLL(path)


class _Fn:
    """what a ctypes function is to the binder: something callable whose restype and argtypes can be set"""
    def __init__(self, value):
        self.value = value

    def __call__(self, *args):
        return self.value


def _stub(key, wrong=None):
    """a library object with every symbol of the table, its version functions answering as expected — but for `wrong`"""
    t = _capi.OPTIONAL_TABLES[key]
    answers = {fn: expected for fn, expected, _ in t["versions"]}
    if wrong:
        answers[wrong] += 1
    return SimpleNamespace(**{"dsr_" + name: _Fn(answers.get(name, 0)) for name in t["signatures"]})


def test_the_registry_lists_every_optional_table():
    assert tuple(_capi.OPTIONAL_TABLES) == KEYS
    tables = [id(t["signatures"]) for t in _capi.OPTIONAL_TABLES.values()]
    assert len(set(tables)) == len(KEYS)
    for key, t in _capi.OPTIONAL_TABLES.items():
        assert t["probe"] in t["signatures"] and t["versions"] and all(fn in t["signatures"] for fn, _, _ in t["versions"]), key


@pytest.mark.parametrize("key", KEYS)
def test_bind_optional_binds_exactly_the_table(lib, key):
    table = _capi.OPTIONAL_TABLES[key]["signatures"]
    ns = _capi.bind_optional(lib, "dsr_", key)
    assert ns is not None and sorted(vars(ns)) == sorted(table)
    for name, (res, args) in table.items():
        fn = getattr(ns, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    legacy = getattr(_capi, "bind_" + key)(lib, "dsr_")
    assert legacy is not None and sorted(vars(legacy)) == sorted(table)


@pytest.mark.parametrize("key", KEYS)
def test_a_library_without_the_probe_symbol_has_no_table(key):
    assert _capi.bind_optional(SimpleNamespace(), "dsr_", key) is None
    assert getattr(_capi, "bind_" + key)(SimpleNamespace(), "dsr_") is None
    full = _stub(key)
    assert _capi.bind_optional(full, "dsr_", key) is not None
    delattr(full, "dsr_" + _capi.OPTIONAL_TABLES[key]["probe"])
    assert _capi.bind_optional(full, "dsr_", key) is None


@pytest.mark.parametrize("key,fn,text", MISMATCHES)
def test_a_wrong_version_is_refused(key, fn, text):
    with pytest.raises(ImportError) as err:
        _capi.bind_optional(_stub(key, wrong=fn), "dsr_", key)
    assert str(err.value) == text
    with pytest.raises(ImportError) as err:
        getattr(_capi, "bind_" + key)(_stub(key, wrong=fn), "dsr_")
    assert str(err.value) == text


def test_one_cache_slot_per_table(lib):
    """Two tables bound through one api object, in either order, never answer for each other (the erase and ESDF bindings once
    shared an attribute of EngineCore, the merge and GC bindings another)."""
    api = _capi.bind(lib, "dsr_")
    first = {key: optional_api(api, key) for key in KEYS}
    for key in reversed(KEYS):
        assert optional_api(api, key) is first[key], key
    assert len({id(ns) for ns in first.values()}) == len(KEYS)
    for key, ns in first.items():
        assert sorted(vars(ns)) == sorted(_capi.OPTIONAL_TABLES[key]["signatures"]), key
    # ... and the other way round on a fresh object: what is asked for first does not decide what a later key gets
    other = _capi.bind(lib, "dsr_")
    for key in reversed(KEYS):
        assert sorted(vars(optional_api(other, key))) == sorted(_capi.OPTIONAL_TABLES[key]["signatures"]), key
        assert optional_api(other, key) is not first[key]


def test_a_backend_without_the_table_is_refused_in_the_existing_words():
    bare = SimpleNamespace(lib=SimpleNamespace(), prefix="orc_")
    for key in KEYS:
        words = "no ICP tracker: dsr_track is a libdsr_hip.so entry point" if key == "track" else f"no include/dsr_{key}.h entry points"
        for _ in range(2):  # (the absence is cached too)
            with pytest.raises(DsrError) as err:
                optional_api(bare, key)
            assert err.value.status == _capi.DSR_E_ARG and str(err.value) == f"dsr status 1: this backend (orc_*) has {words}", key
    with pytest.raises(DsrError) as err:
        optional_api(bare, "esdf", "libdsr_hip.so has no include/dsr_esdf.h entry points")
    assert str(err.value) == "dsr status 1: libdsr_hip.so has no include/dsr_esdf.h entry points"
