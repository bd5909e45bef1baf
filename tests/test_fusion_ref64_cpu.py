"""The CPU oracle's fusion against the float64 statement of tests/fusion_ref64.py, on every case of tests/fusion_cases.py
(DESIGN.md 27): the oracle is what the GPU suite compares the HIP kernels with bit for bit, and this is what pins the oracle
where test_oracle_kat.py's single constant plane cannot see — rotations, a textured colour image, a colour camera of its own."""
import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, InfiniTamDriver
from tests import fusion_cases as fc


def oracle_engine(case):
    from oracle.oracle import OracleEngine, oracle_settings
    return fc.make_engine(OracleEngine, oracle_settings, case)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_oracle_fusion_matches_float64_statement(oracle_lib, case):
    o = oracle_engine(case)
    (replay,) = fc.run_engines([o], case)
    fc.check(case, fc.compare(case, o, replay))


@pytest.mark.parametrize("cam", ["larger", "smaller"])
def test_oracle_colour_image_has_its_own_size(oracle_lib, cam):
    case = (cam, "plain", "float")
    o = oracle_engine(case)
    held, given_d, given_c, rgba = fc.frames(cam, None, "float")[0]
    o.set_view_float(given_c, given_d)
    got, depth = o.get_view()
    assert got.shape == rgba.shape and np.array_equal(got, rgba) and np.array_equal(depth, held)
    img, _ = o.get_image(_capi.IMAGE_ORIGINAL_RGB)
    assert img.shape == rgba.shape and np.array_equal(img, rgba)
    # calls that move whole frames between the two images refuse the engine and leave the view as it was
    mask = np.ones((8, 8), np.uint8)
    for call in (lambda: o.remove_silhouette(mask, 4, 4), lambda: o.extract_silhouette(oracle_engine(case), mask, 4, 4)):
        with pytest.raises(DsrError) as ex:
            call()
        assert ex.value.status == _capi.DSR_E_ARG
    got2, depth2 = o.get_view()
    assert np.array_equal(got2, rgba) and np.array_equal(depth2, held)


def test_drivers_refuse_unequal_sizes(oracle_lib):
    from oracle.oracle import oracle_driver, oracle_settings
    with pytest.raises(DsrError, match="one size"):
        oracle_driver(oracle_settings(**fc.settings_kw("plain")), fc.calib_of("larger"))
    with pytest.raises(DsrError, match="one size"):
        InfiniTamDriver(oracle_settings(**fc.settings_kw("plain")), fc.calib_of("smaller"))
    from dynslam_amd.multigpu import ShardedScene
    made = []

    def make(kind):
        made.append(oracle_engine(("larger", "plain", "float")))
        return made[-1]
    with pytest.raises(DsrError, match="one size"):
        ShardedScene(make, fc.W, fc.H, 1, 1, 0, "cpu", local_only=True, has_static=True)
    assert made and all(e._h is None for e in made), "a refused scene closes the engines it had made"
