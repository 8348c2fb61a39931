"""Depth check of matches, the parts around the kernel that need no device: the host comparison of scripts/depth_verify_bench.py against the
numpy restatement, DepthTemplates.from_mesh with an iterator of views, and a NaN similarity in lmx_cluster_matches."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import depth_verify_cases as dvc
from conftest import ROOT, has_gpu
from linemod_pose_estimation_amd import _lib, meshsynth as ms
from linemod_pose_estimation_amd import MATCH_DTYPE, DepthTemplates, cluster_matches_scored
from linemod_pose_estimation_amd.detector import cluster_matches


@pytest.fixture(scope="module")
def bench_script():
    spec = importlib.util.spec_from_file_location("depth_verify_bench", os.path.join(ROOT, "scripts", "depth_verify_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_script_host_comparison_equals_the_numpy_restatement(bench_script):
    crops, scene, rows, _ = dvc.constructed()
    crops = list(crops) + [np.zeros((0, 0), np.uint16)]
    host = bench_script.HostDiff(crops)
    assert host.ps.tolist() == [(c.shape[1] + 7) // 8 * 8 for c in crops]
    # three frames of different content, the first without matches; every constructed placement once, and the empty crop
    frames = [scene, np.ascontiguousarray(scene[::-1]), np.ascontiguousarray(scene[:, ::-1])]
    half = len(rows) // 2
    m = dvc.match_records(MATCH_DTYPE, np.concatenate([rows, [(3, 4, len(crops) - 1)]]))
    offs = [0, 0, half, len(m)]
    want = dvc.np_diff_matches(crops, frames, m, offs)
    for vectors in (0, 1):
        assert np.array_equal(host(frames, m, offs, vectors), want)
    assert (want[:, 1] > 0).sum() > 500 and want[-1].tolist() == [0, 0, 0]


def test_from_mesh_takes_any_iterable_of_views():
    chip, views = ms.load_mesh("memoryChip2"), ms.view_grid()[:2]
    F = ms.ENSENSO["fx"] / 2
    t = DepthTemplates.from_mesh(chip, zip([], []), 320, 240, F, F)         # no views: no device needed
    assert len(t) == 0
    t.close()
    if has_gpu():
        t = DepthTemplates.from_mesh(chip, iter(views), 320, 240, F, F)
        assert len(t) == 2
        t.close()
    else:
        with pytest.raises(_lib.LmxError) as e:
            DepthTemplates.from_mesh(chip, iter(views), 320, 240, F, F)
        assert e.value.status == _lib.LMX_ERR_NO_DEVICE


def test_nan_similarity_passes_through_cluster_matches_and_is_refused_as_a_value():
    m = dvc.match_records(MATCH_DTYPE, [(10, 10, 0), (11, 10, 0), (12, 11, 0), (200, 200, 0), (201, 200, 0), (202, 201, 0)])
    m["similarity"][1] = np.nan
    dists, rects = [0.5], [[0, 0, 20, 20]]
    clusters, members = cluster_matches(m, dists, rects, 8, 0.4, 0.1)
    assert len(clusters) == 2 and np.isnan(clusters["score"]).sum() == 1
    with pytest.raises(_lib.LmxError) as e:
        cluster_matches_scored(m, m["similarity"].astype(np.float64), dists, rects, 8, 0.4, 0.1)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "not a number" in str(e.value)
