"""The big sort of the large-frame chain (csrc/lmx_sort_block.hpp at 16384 elements and 1024 threads, keys and tags in device memory, as
k_f2_large runs it) against the REAL std::sort through lmx_debug_device_sort_perm_large: the same permutation, ties included.  Sizes on
both sides of the leaf size 16, of the LDS kernels' 2048, of a power of two and of the limit 16384; input kinds that give balanced trees,
one-sided trees and -- the median-of-three killers -- a tree that reaches the depth limit, where the kernel heap-sorts the remaining ranges on
the device (the choice DESIGN.md section 7 states: no hand-back status), so the killers must give std::sort's permutation too."""
import numpy as np
import pytest

import cluster_cases as cc
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd.detector import F2_LARGE_MAX
from test_sort_emulation import median_of_three_killer

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 16, 17, 2048, 2049, 4095, 4096, 4097, 16383, 16384)


def device_perm(sim, tid):
    sim = np.ascontiguousarray(sim, np.float32)
    tid = np.ascontiguousarray(tid, np.int32)
    perm = np.full(len(sim), -1, np.int32)
    _lib.check(_lib.lib().lmx_debug_device_sort_perm_large(0, sim.ctypes.data, tid.ctypes.data, len(sim), perm.ctypes.data))
    return perm


def check(sim, tid, what):
    a, b = cc.std_sort_perm(sim, tid), device_perm(sim, tid)
    assert np.array_equal(a, b), (what, len(a), np.flatnonzero(a != b)[:5], a[:8], b[:8])


@pytest.mark.parametrize("n", SIZES)
def test_large_block_sort_equals_std_sort(n):
    rng = np.random.default_rng(9000 + n)
    idx = np.arange(n)
    zeros = np.zeros(n, np.int32)
    for levels, tids in ((1, 1), (3, 50), (10, 5), (40, 3000), (10 ** 6, 3000)):
        check(rng.integers(0, levels, n).astype(np.float32) * 0.25 + 90, rng.integers(0, tids, n), ("random", levels, tids))
    check(np.full(n, 95.0), zeros, "all equal")
    check(-idx.astype(np.float32), zeros, "sorted")
    check(idx.astype(np.float32), zeros, "reversed")
    check(np.full(n, 95.0), idx[::-1], "reversed by template")
    check(np.minimum(idx, n - 1 - idx).astype(np.float32), zeros, "organ pipe")


@pytest.mark.parametrize("n", (2049, 4096, 16384))
def test_median_of_three_killers_reach_the_depth_limit_and_still_sort_as_std_sort(n):
    idx = np.arange(n)
    check(np.full(n, 95.0), median_of_three_killer(n), "killer by template")
    check(-median_of_three_killer(n).astype(np.float32), idx % 3, "killer by similarity")


def test_more_than_16384_elements_are_refused():
    n = F2_LARGE_MAX + 1
    sim, tid, perm = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    st = _lib.lib().lmx_debug_device_sort_perm_large(0, sim.ctypes.data, tid.ctypes.data, n, perm.ctypes.data)
    assert st == _lib.LMX_ERR_INVALID_ARG
