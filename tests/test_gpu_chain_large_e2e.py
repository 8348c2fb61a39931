"""lmx_ctx_collect_clusters, _depth and _classes on batches with a frame of more than 2048 raw records: the large-frame kernel completes it
inside the call (Detector.chain_stats says so), the result equals the oracle's / the composition's; with LMX_F2_LARGE=0 in the environment
of the context's creation the host completes it as before, with the same result.  The configurations are those of the three existing
host-fallback tests (160 x 160, bank seed 91, scenes 94 / 93, threshold 45).  The context exposes no accounting of its device allocations,
so "a context that only sees small frames allocates nothing for the large path" is asserted on chain_stats()'s large_workspace_bytes."""
from types import SimpleNamespace

import numpy as np
import pytest

import cluster_cases as cc
import cluster_class_cases as ccc
import depth_verify_cases as dvc
import test_gpu_cluster_classes as tgc
import test_gpu_cluster_depth as tgd
from linemod_pose_estimation_amd import DepthTemplates, Detector, cluster_matches_scored, depth_values, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

S, THR = 160, 45.0
PART_BYTES = {"similarity": 2457600, "depth": 2719744}     # one large frame's part of the workspace (csrc/lmx_internal.hpp: f2_large_layout)


def scenes_of(bank):
    return [synth.make_scene(bank, S, S, seed=94)[0], synth.make_scene(bank, S, S, seed=93, n_instances=1)[0]]


def raw_sizes(bank, frames):
    od = o.OracleDetector(bank)
    sizes = []
    for fr in frames:
        od.match(fr, THR)
        sizes.append(len(od.last_raw()))
    assert cc.F2_MAX < sizes[0] <= 16384 and cc.F2_MAX > sizes[1] > 0, sizes      # frame 0 is a large frame, frame 1 an LDS frame
    return sizes


def check_stats(st, large, sizes, part_bytes):
    want = {"frames": 2, "frames_lds": 1, "frames_large": 1 if large else 0, "frames_host_records": 0 if large else 1, "frames_host_other": 0,
            "max_frame_records": sizes[0], "large_workspace_bytes": part_bytes if large else 0}
    assert st == want, (st, want)


@pytest.fixture(params=[True, False], ids=["large_kernel", "LMX_F2_LARGE=0"])
def large(request, monkeypatch):
    if not request.param:
        monkeypatch.setenv("LMX_F2_LARGE", "0")      # read when a context is created
    return request.param


def test_collect_clusters_with_a_large_frame(large):
    n_t = 80
    bank = synth.make_bank(n_t, seed=91, size_range=(20.0, 36.0))
    frames = scenes_of(bank)
    sizes = raw_sizes(bank, frames)
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(n_t) % 4) + rng.uniform(-0.005, 0.005, n_t)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    od = o.OracleDetector(bank)
    det = Detector(bank, S, S, max_batch=2, max_candidates=1 << 17)
    det.set_cluster_sidecar(dists, rects, 10, 0.5, 0.1, 2)
    # the small frame alone first: nothing is allocated for the large path
    det.upload(frames[1:])
    det.enqueue(1, THR)
    det.collect_clusters(1)
    st = det.chain_stats()
    assert st["frames"] == st["frames_lds"] == 1 and st["frames_large"] == 0 and st["max_frame_records"] == 0 and st["large_workspace_bytes"] == 0, st
    det.upload(frames)
    det.enqueue(2, THR)
    got = det.collect_clusters(2, cap_total=1 << 17)
    check_stats(det.chain_stats(), large, sizes, PART_BYTES["similarity"])
    for f in range(2):
        ref_m = od.match(frames[f], THR)
        ref_c, ref_mem = o.cluster_matches(ref_m, dists, rects, 10, 0.5, 0.1, 2)
        m, c, mem = got[f]
        assert len(m) == len(ref_m)
        for k in cc.FIELDS:
            assert np.array_equal(m[k], ref_m[k]), (f, k)
        assert len(c) == len(ref_c) > 0, (f, len(c), len(ref_c))
        for k in ("index", "rect", "score", "member_count"):
            assert np.array_equal(c[k], ref_c[k]), (f, k)
        for a, b in zip(c, ref_c):
            assert np.array_equal(mem[a["member_begin"]:a["member_begin"] + a["member_count"]], ref_mem[b["member_begin"]:b["member_begin"] + b["member_count"]])
    det.close()


def test_collect_clusters_depth_with_a_large_frame(large):
    n_t = 80
    bank = synth.make_bank(n_t, seed=91, size_range=(20.0, 36.0))
    frames = scenes_of(bank)
    sizes = raw_sizes(bank, frames)
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(n_t) % 4) + rng.uniform(-0.005, 0.005, n_t)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    crops = [dvc._values(rng, (int(r[3]), int(r[2])), 0.3) for r in rects]
    depth = [np.ascontiguousarray(fr[1]) for fr in frames]
    t = DepthTemplates.from_crops(crops)
    det = Detector(bank, S, S, max_batch=2, max_candidates=1 << 17)
    det.set_cluster_sidecar(dists, rects, 10, 0.5, 0.1, 2)
    det.upload(frames)
    det.enqueue(2, THR)
    det.enqueue(2, THR)
    per_frame = det.collect(2, cap_total=1 << 17)
    t.upload_scene(depth)
    got = det.collect_clusters_depth(2, t, cap_total=1 << 17)
    check_stats(det.chain_stats(), large, sizes, PART_BYTES["depth"])
    for f in range(2):
        d = t.diff(depth[f], per_frame[f])
        assert (d["n_valid"] > 0).any()
        c, mem = cluster_matches_scored(per_frame[f], depth_values(d), dists, rects, 10, 0.5, 0.1, 2)
        assert len(c) > 0
        tgd.assert_frame_equals_composition(got[f], per_frame[f], d, c, mem, what=f)
    t.close()
    det.close()


def test_collect_clusters_classes_with_a_large_frame(large):
    n_t = 40
    bank = synth.make_bank(n_t, seed=91, size_range=(20.0, 36.0), classes=["a", "b"])
    frames = scenes_of(bank)
    sizes = raw_sizes(bank, frames)
    depth = [np.ascontiguousarray(fr[1]) for fr in frames]
    det = Detector(bank, S, S, max_batch=2, max_candidates=1 << 17)
    by_name = {cid: t for cid, t, _ in bank.classes}
    rows = len(bank.T) * len(bank.modalities)
    rng = np.random.default_rng(8)
    tc = SimpleNamespace(det=det, depth=depth, classes=[], crops=[])
    for c, cid in enumerate(det.classIds()):
        tm = by_name[cid][::rows]
        n = len(tm)
        rects = np.stack([np.zeros(n), np.zeros(n), tm[:, 0], tm[:, 1]], 1).astype(np.int32)
        dists = 0.5 + 0.1 * ((np.arange(n) + c) % 4) + rng.uniform(-0.005, 0.005, n)
        tc.classes.append(ccc.Side(dists, rects, 10, 0.5, 0.1, 2))
        tc.crops.append([tgc.ramp((int(r[3]), int(r[2])), int(rng.integers(600, 1400))) for r in rects])
        det.set_cluster_sidecar_class(c, dists, rects, 10, 0.5, 0.1, 2)
    t = tgc.joined_object(tc.crops, False)
    det.upload(frames)
    for mode in ("similarity", "depth"):
        det.enqueue(2, THR)
        det.enqueue(2, THR)
        per_frame = det.collect(2, cap_total=1 << 17)
        want = tgc.e2e_composition(tc, per_frame, mode)
        if mode == "similarity":
            got = det.collect_clusters_classes(2, cap_total=1 << 17)
        else:
            t.upload_scene(depth)
            got = det.collect_clusters_classes(2, t, tgc.class_base_of(tc.crops), cap_total=1 << 17)
        check_stats(det.chain_stats(), large, sizes, PART_BYTES[mode])     # the workspace grows from the unscored to the scored layout
        for f in range(2):
            assert len(want[f][3]) > 0 and set(want[f][4].tolist()) == {0, 1}
            tgc.assert_frame(got[f], want[f], (mode, f))
    t.close()
    det.close()
