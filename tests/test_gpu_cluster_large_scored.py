"""The scored and the per-class instantiations of the large-frame chain (k_f2_large with a score, with classes, and with both)
through lmx_debug_device_finalize_cluster_large_depth and _large_classes, on two frames of 2049 and 4096 records from the lattice builders
of tests/cluster_cases.py.  Expected values: the cases' library-independent final matches, then the host composition the scored tests of
the LDS kernels use -- lmx_depth_diff_matches / lmx_normal_diff_matches on those matches and lmx_cluster_matches_scored, per class for the
classed forms (tests/test_gpu_cluster_classes.py: per_class_diffs, composition).  Everything is compared bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest

import cluster_cases as cc
import cluster_class_cases as ccc
import test_gpu_cluster_classes as tgc
import test_gpu_cluster_depth as tgd
from linemod_pose_estimation_amd import DEPTH_DIFF_DTYPE, MATCH_DTYPE, DepthTemplates, cluster_matches_scored
from linemod_pose_estimation_amd.detector import debug_device_finalize_cluster_large_classes, debug_device_finalize_cluster_large_depth

pytestmark = pytest.mark.gpu

SIZES = (2049, 4096)


def with_repeats(rng, r, share=0.1):
    """A share of exact repeats of (x, y, similarity, template, class): what std::unique removes where they end up adjacent."""
    k = rng.integers(0, len(r), int(len(r) * share))
    src = rng.integers(0, len(r), len(k))
    for fld in cc.FIELDS:
        r[fld][k] = r[fld][src]
    return r


# ---- un-classed, depth score ---------------------------------------------------------------------------------------------------------------
def depth_case():
    rng = np.random.default_rng(401)
    dists, rects = cc.sidecar(rng, 12)
    parts = [cc.draw_frame(rng, f, n, 12, cc.SIMS[:3], grid=(4, 3), pitch=20, n_cls=1, dup=0.1) for f, n in enumerate(SIZES)]
    case = cc.Case("large_depth", cc.interleave(rng, parts), 2, dists, rects, 10, thresh=2)
    ref = cc.reference(case)
    assert [r.n_records for r in ref] == list(SIZES) and all(r.n_records > len(r.matches) > 1000 and len(r.clusters) > 3 for r in ref)
    return case


def test_depth_scored_frames_on_the_large_kernel():
    case = depth_case()
    ref = cc.reference(case)
    crops, scenes = tgd.make_crops(len(case.dists), 510), tgd.make_scenes(2, 610)
    t = DepthTemplates.from_crops(crops)
    try:
        flat = np.ascontiguousarray(np.concatenate([r.matches for r in ref])).astype(MATCH_DTYPE)
        offsets = np.concatenate([[0], np.cumsum([len(r.matches) for r in ref])])
        dd = t.diff(scenes, flat, offsets)                                       # lmx_depth_diff_matches
        assert (dd["n_valid"] > 0).any() and (dd["n_template"] == 0).any()       # something to score, and the empty crops
        got, counts = debug_device_finalize_cluster_large_depth(case.records, 2, t, scenes, case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh,
                                                                with_counts=True)
    finally:
        t.close()
    orders = []
    for f, r in enumerate(ref):
        m, d, c, mem, status = got[f]
        e_d = dd[offsets[f]:offsets[f + 1]]
        e_c, e_mem = cluster_matches_scored(flat[offsets[f]:offsets[f + 1]], tgd.values_of(e_d, -np.inf), case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)
        e_mem = e_mem[:int(e_c["member_count"].sum())]
        assert status == 0 and counts[f].tolist() == [len(r.matches), len(e_c), len(e_mem), 0], (f, counts[f].tolist())
        for k in cc.FIELDS:
            assert np.array_equal(m[k], r.matches[k]), (f, k)
        for k in DEPTH_DIFF_DTYPE.names:
            assert np.array_equal(d[k], e_d[k]), (f, k)
        for k in cc.CLUSTER_FIELDS:
            assert np.array_equal(c[k], e_c[k]), (f, k)
        assert c["score"].tobytes() == e_c["score"].tobytes() and np.array_equal(mem, e_mem), f
        orders.append(([tuple(i) for i in e_c["index"]], [tuple(i) for i in r.clusters["index"]]))
    assert any(a != b for a, b in orders)      # the depth score ranks otherwise than the mean similarity: the scored instantiation ran


# ---- per class: no score, depth score, depth + normal score ------------------------------------------------------------------------------
def class_case():
    """Three classes: 0 with a side-car, 1 without (listed, in no cluster), 2 with another side-car and with most of the records -- alone
    more than 2048 in the second frame."""
    rng = np.random.default_rng(402)
    da, ra = cc.sidecar(rng, 9)
    db, rb = cc.sidecar(rng, 9, rings=2)
    parts = []
    for f, n in enumerate(SIZES):
        r = cc.draw_frame(rng, f, n, 9, cc.SIMS[:3], grid=(3, 2), pitch=16, n_cls=1, dup=0.0)
        r["class_index"] = rng.choice([0, 1, 2], n, p=[0.2, 0.12, 0.68])
        parts.append(with_repeats(rng, r))
    case = ccc.ClassCase("large_classes", cc.interleave(rng, parts), 2, [ccc.Side(da, ra, 8, thresh=2), None, ccc.Side(db, rb, 10, 0.45, 0.1, 1)])
    ref = ccc.reference(case)
    assert [r.n_records for r in ref] == list(SIZES)
    assert (ref[1].matches["class_index"] == 2).sum() > 2048
    for r in ref:
        assert r.n_records > len(r.matches) > 1000 and set(r.cluster_class.tolist()) == {0, 2} and (r.matches["class_index"] == 1).sum() > 100
        assert (r.matches["class_index"][r.members] != 1).all()
    return case


def expected_classes(case, mode):
    """tests/test_gpu_cluster_classes.py's `expected` with every frame complete (its status rule is the LDS kernels')."""
    ref = ccc.reference(case)
    diffs = tgc.per_class_diffs(tgc.crops_of(case), tgc.scenes_of(case), [r.matches for r in ref], mode == "normal") if mode != "similarity" else None
    out = []
    for f, r in enumerate(ref):
        e = SimpleNamespace(status=0, n_records=r.n_records, matches=r.matches, dd=None, nd=None)
        if diffs is None:
            e.clusters, e.cluster_class, e.members = r.clusters, r.cluster_class, r.members
        else:
            e.dd, e.nd = diffs[f]
            e.clusters, e.cluster_class, e.members = tgc.composition(case.classes, r.matches, tgc.values_of(e.dd, e.nd, -np.inf))
        out.append(e)
    return out


@pytest.mark.parametrize("mode", tgc.MODES)
def test_classed_frames_on_the_large_kernel(mode, monkeypatch):
    case = class_case()
    want = expected_classes(case, mode)
    if mode != "similarity":
        assert all((e.dd["n_valid"] > 0).any() for e in want) and (mode == "depth" or all((e.nd["n_normal"] > 0).any() for e in want))
    monkeypatch.setattr(tgc, "debug_device_finalize_cluster_classes", debug_device_finalize_cluster_large_classes)   # run_hook's hook
    tgc.check_hook(case, mode, want)
