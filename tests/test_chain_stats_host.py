"""lmx_ctx_chain_stats and the large-frame test hooks where no GPU is needed: argument checks, LMX_ERR_NO_DEVICE without a device, the
Python mirrors."""
import ctypes as C

import numpy as np

import linemod_pose_estimation_amd.detector as det
from conftest import has_gpu
from linemod_pose_estimation_amd import Detector, _lib


def test_chain_stats_refuses_null_arguments():
    L = _lib.lib()
    s = _lib.ChainStats()
    assert L.lmx_ctx_chain_stats(None, C.byref(s)) == _lib.LMX_ERR_INVALID_ARG
    assert "lmx_ctx_chain_stats" in L.lmx_last_error().decode()
    assert L.lmx_ctx_chain_stats(None, None) == _lib.LMX_ERR_INVALID_ARG
    assert [k for k, _ in _lib.ChainStats._fields_] == ["frames", "frames_lds", "frames_large", "frames_host_records", "frames_host_other", "max_frame_records",
                                                         "large_workspace_bytes"]
    assert C.sizeof(_lib.ChainStats) == 32


def test_large_hooks_report_no_device_without_a_gpu():
    L = _lib.lib()
    sim, tid, perm = np.zeros(4, np.float32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    # argument checks come before the device is looked for
    assert L.lmx_debug_device_sort_perm_large(0, sim.ctypes.data, tid.ctypes.data, det.F2_LARGE_MAX + 1, perm.ctypes.data) == _lib.LMX_ERR_INVALID_ARG
    assert L.lmx_debug_device_sort_perm_large(0, None, None, 4, None) == _lib.LMX_ERR_INVALID_ARG
    if has_gpu():       # the rest is what a machine without a device answers
        return
    assert L.lmx_debug_device_sort_perm_large(0, sim.ctypes.data, tid.ctypes.data, 4, perm.ctypes.data) == _lib.LMX_ERR_NO_DEVICE
    rec = np.zeros(3, det.RAW_MATCH_DTYPE)
    rows = det.F2_LARGE_MAX
    m, cl, mem, counts = np.zeros(rows, det.MATCH_DTYPE), np.zeros(rows, det.CLUSTER_DTYPE), np.zeros(rows, np.int32), np.zeros(4, np.uint32)
    dists, rects = np.array([0.7]), np.array([[0, 0, 10, 10]], np.int32)
    pp = _lib.ClusterParams(10, 0.5, 0.1, 2)
    st = L.lmx_debug_device_finalize_cluster_large(0, rec.ctypes.data, 3, 1, dists.ctypes.data, rects.ctypes.data, 1, C.byref(pp), m.ctypes.data, cl.ctypes.data,
                                                   mem.ctypes.data, counts.ctypes.data)
    assert st == _lib.LMX_ERR_NO_DEVICE
    side = _lib.ClassSidecar(dists.ctypes.data, rects.ctypes.data, 1, pp)
    k = np.zeros(rows, np.int32)
    st = L.lmx_debug_device_finalize_cluster_large_classes(0, rec.ctypes.data, 3, 1, C.byref(side), 1, None, None, m.ctypes.data, None, None, cl.ctypes.data, k.ctypes.data,
                                                           mem.ctypes.data, counts.ctypes.data)
    assert st == _lib.LMX_ERR_NO_DEVICE


def test_python_mirrors_exist():
    assert det.F2_MAX == 2048 and det.F2_LARGE_MAX == 16384
    for name in ("debug_device_finalize_cluster_large", "debug_device_finalize_cluster_large_depth", "debug_device_finalize_cluster_large_classes"):
        assert callable(getattr(det, name))
    assert callable(Detector.chain_stats)
    L = _lib.lib()
    for name in ("lmx_ctx_chain_stats", "lmx_debug_device_sort_perm_large", "lmx_debug_device_finalize_cluster_large", "lmx_debug_device_finalize_cluster_large_depth",
                 "lmx_debug_device_finalize_cluster_large_classes"):
        assert hasattr(L, name)
