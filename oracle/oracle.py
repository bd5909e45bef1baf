"""ctypes binding of the CPU oracle (oracle/liboracle.so, prefix `orc_`).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg, never by the product (dynslam_amd/).
"""
import ctypes as C
import os
import subprocess

from dynslam_amd import _capi
from dynslam_amd.engine import EngineCore, InfiniTamDriver, default_settings  # noqa: F401 (re-export)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboracle.so")
_api = None


def build(force=False):
    src = os.path.join(_HERE, "dsr_oracle.cpp")
    hdr = os.path.join(_HERE, "..", "include", "dsr.h")
    stale = (not os.path.exists(LIB_PATH)
             or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(src), os.path.getmtime(hdr),
                                                  os.path.getmtime(os.path.join(_HERE, "mc_tables.h"))))
    if force or stale:
        subprocess.check_call(["make", "-C", _HERE, "-B", "liboracle.so"], stdout=subprocess.DEVNULL)


def load_api():
    global _api
    if _api is None:
        if not os.path.exists(LIB_PATH):
            build()
        lib = C.CDLL(LIB_PATH)
        _api = _capi.bind(lib, "orc_")
        _api.set_threads = lib.orc_set_threads
        _api.set_threads.restype = C.c_int
        _api.set_threads.argtypes = [C.c_void_p, C.c_int]
        _api.set_scene_state = lib.orc_set_scene_state
        _api.set_scene_state.restype = C.c_int
        _api.set_scene_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64]
    return _api


def oracle_settings(**overrides):
    return default_settings(api=load_api(), **overrides)


class OracleEngine(EngineCore):
    def __init__(self, settings, calib, threads=1):
        super().__init__(settings, calib, api=load_api())
        if threads != 1:
            self.set_threads(threads)

    def set_threads(self, n):
        self._check(self.api.set_threads(self._h, int(n)))

    def set_scene_state(self, state):
        """Take on the scene state an edit call left (orc_set_scene_state); `state`: a dict as tests/erase_util.state() produces —
        table, voxels, val / lfb, exl / lfe, vis, vis_types, decayed.  The oracle has no merge, import or erase of its own: their
        serial restatements compute the state, this hook lets the oracle go on from it."""
        import numpy as np
        from dynslam_amd.engine import HASH_ENTRY_DTYPE, VOXEL_DTYPE
        table = np.ascontiguousarray(state["table"], HASH_ENTRY_DTYPE)
        voxels = np.ascontiguousarray(state["voxels"], VOXEL_DTYPE).reshape(-1)
        val, exl = np.ascontiguousarray(state["val"], np.int32), np.ascontiguousarray(state["exl"], np.int32)
        vis, vt = np.ascontiguousarray(state["vis"], np.int32), np.ascontiguousarray(state["vis_types"], np.uint8)
        nblk, rem = divmod(voxels.size, 512)
        self._check(self.api.set_scene_state(self._h, table.ctypes.data, table.size, voxels.ctypes.data, nblk if rem == 0 else -1,
                                             val.ctypes.data, val.size, int(state["lfb"]), exl.ctypes.data, exl.size, int(state["lfe"]),
                                             vis.ctypes.data if vis.size else None, vis.size, vt.ctypes.data, vt.size,
                                             int(state["decayed"])))


def oracle_driver(settings, calib, voxel_decay_params=None, use_depth_weighting=False):
    """An InfiniTamDriver mirror running on the oracle."""
    return InfiniTamDriver(settings, calib, voxel_decay_params, use_depth_weighting, api=load_api())
