"""lmx_ctx_export_clusters_on through Detector.export_clusters: the clusters of all six chains (un-classed / per class, times mean similarity /
depth / depth + normal) left in device memory, and the kernel it adds, k_walk_records_dev (csrc/lmx_verify.hip): the crop walk over the
slot's raw records by persistent workgroups that read the record count from device memory.
Yardsticks, all of them entry points and restatements that existed before: collect_clusters, collect_clusters_depth,
collect_clusters_depth_normal and collect_clusters_classes of the SAME enqueue after the export (the export consumes nothing);
depth_verify_cases.np_diff per record and DepthTemplates.normal_diff (the job form of k_walk) for the walk alone.  Everything is compared bit for bit.
Configurations: tests/test_gpu_export_matches.py's (160 x 160, bank seed 91, 80 templates, threshold 45: frame A beyond 2048 raw records,
Z none, B few) with one crop per template, and tests/test_gpu_cluster_classes.py's two-class fixture.
Not reached: a frame beyond 16384 records and a device group's member context, as in tests/test_gpu_export_matches.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cluster_cases as cc
import depth_verify_cases as dvc
from linemod_pose_estimation_amd import (DEPTH_DIFF_DTYPE, MATCH_DTYPE, NORMAL_DIFF_DTYPE, DepthTemplates, Detector, ExportedClusters, PinnedArena, _lib, synth)
from linemod_pose_estimation_amd import detector as D
from test_gpu_cluster_classes import E2E, class_base_of, joined_object, ramp, two_classes  # noqa: F401  (two_classes is a fixture)
from test_gpu_cluster_depth import make_crops

pytestmark = pytest.mark.gpu

S, THR, N_T = 160, 45.0, 80
SIDE = (10, 0.5, 0.1, 2)
FX = FY = 520.0
CANARY = 0x5a
SCORES = (0, 1, 2)


# ---- 1. the walk alone ---------------------------------------------------------------------------------------------------------------------------
WALK_W, WALK_H, WALK_FRAMES = 96, 80, 2
WALK_BASE = (0, 8, 16)          # the classed variants: class 0 holds crops 0 .. 7, class 1 crops 8 .. 15


def walk_records():
    """54 records that mix jobs with every kind of non-job, and per variant the crop each is walked against (None: no job)"""
    rng = np.random.default_rng(2025)
    n = 54
    rec = np.zeros(n, D.RAW_MATCH_DTYPE)
    kind = rng.choice(6, n, p=[0.5, 0.1, 0.1, 0.1, 0.1, 0.1])      # 0 job, 1 class 1, 2 class 2, 3 template outside the table, 4 frame outside, 5 empty crop
    kind[:9] = [0, 0, 2, 0, 5, 0, 3, 4, 0]                          # job -> job, job -> non-job -> job, job -> empty crop -> job
    # ... and the same three for a workgroup that takes every second or every third record
    for first, mid in ((14, 0), (20, 5), (40, 2)):
        kind[[first, first + 2, first + 4]] = [0, mid, 0]
    for first, mid in ((15, 0), (30, 5), (45, 2)):
        kind[[first, first + 3, first + 6]] = [0, mid, 0]
    kind[[46, 48, 50, 52]] = [0, 2, 2, 0]                           # two non-jobs between two jobs of an every-second-record workgroup
    for i in range(n):
        k = int(kind[i])
        tid = int(rng.choice([0, 1, 2, 3, 4, 6, 7])) if k != 5 else 5
        cls = {1: 1, 2: 2}.get(k, 0)
        if k == 1:
            tid = int(rng.choice([0, 3, 4, 6, 7, 9]))                # class 1: crops 8, 11, 12 (empty), 14, 15 (ramps); 9 is outside its range
        if k == 3:
            tid = int(rng.choice([16, 40, -1]))
        rec[i] = (int(rng.integers(-20, WALK_W + 4)), int(rng.integers(-6, WALK_H + 2)), 80.0, tid, cls, int(rng.choice([2, -1, 7])) if k == 4 else i % 2, i)
    # jobs of the two ramp crops where the scene is a ramp too (normals on both sides): through class 1 for the classed variants, by
    # their index in the table for the un-classed ones
    rec[9], rec[10] = (10, 30, 80.0, 6, 1, 1, 9), (20, 40, 80.0, 7, 1, 1, 10)
    rec[11], rec[12] = (10, 30, 80.0, 14, 0, 1, 11), (20, 40, 80.0, 15, 0, 1, 12)

    def crop_of(r, classes):
        tid, cls, fr = int(r["template_id"]), int(r["class_index"]), int(r["frame"])
        if not 0 <= fr < WALK_FRAMES:
            return None
        if classes:
            if not 0 <= cls < 2 or not 0 <= tid < WALK_BASE[cls + 1] - WALK_BASE[cls]:
                return None
            return WALK_BASE[cls] + tid
        return tid if cls == 0 and 0 <= tid < WALK_BASE[2] else None

    return rec, {classes: [crop_of(r, classes) for r in rec] for classes in (False, True)}


@pytest.fixture(scope="module")
def walk():
    """16 crops (14 of make_crops: 8 to 129 columns, a few rows, crops 5 and 12 empty; two ramps tall enough for normals), two 96 x 80
    scenes, walk_records(), and the expected sums per record for the four variants."""
    rng = np.random.default_rng(2026)
    crops = make_crops(14, 3) + [ramp((13, 15), 700), ramp((12, 64), 760)]
    scenes = [dvc._values(rng, (WALK_H, WALK_W), 0.2), ramp((WALK_H, WALK_W), 690)]
    scenes[1][20:24, 30:40] = 0
    t = DepthTemplates.from_crops(crops)
    t.enable_normals(FX, FY)
    rec, all_ids = walk_records()
    n = len(rec)
    want = {}
    for classes in (False, True):
        ids = all_ids[classes]
        dd = np.zeros(n, DEPTH_DIFF_DTYPE)
        for i, k in enumerate(ids):
            if k is not None and crops[k].size:
                dd[i] = dvc.np_diff(crops[k], scenes[int(rec["frame"][i])], int(rec["x"][i]), int(rec["y"][i]))
        # the one-workgroup-per-item kernels on the jobs: k_walk through normal_diff, frame by frame
        nd = np.zeros(n, NORMAL_DIFF_DTYPE)
        jobs = [i for i, k in enumerate(ids) if k is not None]
        order = sorted(jobs, key=lambda i: int(rec["frame"][i]))
        m = np.zeros(len(order), MATCH_DTYPE)
        for j, i in enumerate(order):
            m[j] = (rec["x"][i], rec["y"][i], 80.0, ids[i], 0)
        offs = [0] + [int(np.sum(rec["frame"][order] <= f)) for f in range(WALK_FRAMES)]
        old_dd, old_nd = t.normal_diff(scenes, m, offs)
        assert np.array_equal(old_dd, dd[order])                     # np_diff and the old kernel agree before the new one is asked
        nd[order] = old_nd
        want[classes] = SimpleNamespace(ids=ids, dd=dd, nd=nd)
        assert (dd["n_valid"] > 0).sum() >= 10 and (nd["n_normal"] > 0).sum() >= 2, classes
    t.upload_scene(scenes)                                            # normal_diff forgot the scene
    yield SimpleNamespace(t=t, rec=rec, n=n, crops=crops, want=want)
    t.close()


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_the_record_list_holds_what_it_is_for(walk, grid):
    """in some workgroup of each grid: two jobs in a row, a job after one and after two non-jobs after a job, a job after an empty crop after a job;
    records partly outside the scene"""
    for classes in (False, True):
        ids = walk.want[classes].ids
        kinds = ["n" if k is None else ("e" if not walk.crops[k].size else "j") for k in ids]
        seqs = ["".join(kinds[b::grid]) for b in range(grid)]
        for pattern in ("jj", "jnj", "jnnj", "jej"):
            assert any(pattern in seq for seq in seqs), (classes, grid, pattern, seqs)
    x, y = walk.rec["x"], walk.rec["y"]
    assert (x < 0).any() and (y < 0).any() and (x > WALK_W - 8).any()


@pytest.mark.parametrize("classes", [False, True])
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("grid", [1, 2, 3, 64])
def test_walk_equals_np_diff_and_the_old_kernels(walk, grid, normals, classes):
    w, n = walk.want[classes], walk.n
    kw = dict(class_base=WALK_BASE) if classes else dict(class_index=0)
    dd, nd = walk.t.debug_walk_records(walk.rec, n, n, n, grid, normals=normals, fill=CANARY, **kw)          # header_count == n_candidates == cap
    assert dd.tobytes() == w.dd.tobytes(), (grid, normals, classes, np.nonzero(dd != w.dd)[0])
    if normals:
        assert nd.tobytes() == w.nd.tobytes(), (grid, classes, np.nonzero(nd != w.nd)[0])
    else:
        assert nd is None


@pytest.mark.parametrize("classes", [False, True])
def test_walk_header_decides_what_is_written(walk, classes):
    w, n = walk.want[classes], walk.n
    kw = dict(class_base=WALK_BASE) if classes else dict(class_index=0)
    canary_d = np.full(n * DEPTH_DIFF_DTYPE.itemsize, CANARY, np.uint8).tobytes()

    def run(header_count, n_cand, cap):
        dd, nd = walk.t.debug_walk_records(walk.rec, header_count, n_cand, cap, 2, normals=True, fill=CANARY, **kw)
        return dd.tobytes(), nd.tobytes()

    for args in ((0, 0, n), (n + 1, 0, n), (3, n + 1, n), (1 << 31, 5, 1 << 20)):      # nothing counted; either list overflowed
        assert run(*args) == (canary_d, canary_d), args
    k = 17                                                                              # fewer records than the list holds: the rest stays
    dd, nd = run(k, 2 * k, 1 << 17)
    cut = k * DEPTH_DIFF_DTYPE.itemsize
    assert dd[:cut] == w.dd[:k].tobytes() and nd[:cut] == w.nd[:k].tobytes() and dd[cut:] == canary_d[cut:] and nd[cut:] == canary_d[cut:]
    # an un-classed walk over every class, and a header that counts more records than were passed
    if not classes:
        dd, _ = walk.t.debug_walk_records(walk.rec, n, n, n, 3, class_index=-1)
        other = np.array([int(c) != 0 and 0 <= int(t) < len(walk.crops) and 0 <= int(f) < WALK_FRAMES for c, t, f in zip(walk.rec["class_index"], walk.rec["template_id"], walk.rec["frame"])])
        assert dd[~other].tobytes() == w.dd[~other].tobytes() and (dd[other]["n_template"] > 0).any()
        with pytest.raises(_lib.LmxError):
            walk.t.debug_walk_records(walk.rec, n + 1, 0, n + 1, 2)


# ---- 2. end to end, un-classed -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg():
    bank = synth.make_bank(N_T, seed=91, size_range=(20.0, 36.0))
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(N_T) % 4) + rng.uniform(-0.005, 0.005, N_T)
    rects = np.stack([np.zeros(N_T), np.zeros(N_T), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    frames = {"A": synth.make_scene(bank, S, S, seed=94)[0], "B": synth.make_scene(bank, S, S, seed=93, n_instances=1)[0],
              "Z": [np.full((S, S, 3), 90, np.uint8), np.full((S, S), 800, np.uint16)]}
    dev, scene, alt = {}, {}, {}
    for k, fr in frames.items():
        fr = [np.ascontiguousarray(s) for s in fr]
        dev[k] = [torch.from_numpy(fr[0]).cuda(), torch.from_numpy(fr[1].view(np.int16)).cuda()]
        scene[k] = dev[k][1].clone()
        alt[k] = torch.from_numpy(np.ascontiguousarray(np.roll(fr[1], (11, 5), (0, 1))).view(np.int16)).cuda()      # a different scene for the same frames
    det = Detector(bank, S, S, max_batch=3, max_candidates=1 << 17)
    det.set_cluster_sidecar(dists, rects, *SIDE)
    crops = make_crops(N_T, 31)
    t = DepthTemplates.from_crops(crops)
    t.enable_normals(FX, FY)
    yield SimpleNamespace(bank=bank, dists=dists, rects=rects, dev=dev, scene=scene, alt=alt, det=det, t=t, crops=crops, cache={})
    t.close()
    det.close()


def upload_enqueue(cfg, names, det=None, stream=None):
    det = det or cfg.det
    det.upload_device([cfg.dev[k] for k in names], stream=stream)
    det.enqueue(len(names), THR)


def scene_of(cfg, names, alt=False):
    return [(cfg.alt if alt else cfg.scene)[k] for k in names]


def export(cfg, n, score, det=None, t=None, **kw):
    kw.setdefault("max_large_frames", 1)
    return (det or cfg.det).export_clusters(n, templates=(t or cfg.t) if score else None, normals=score == 2, **kw)


def collect(cfg, n, score, det=None, t=None):
    """the matching collect call -> per frame (matches, diffs, ndiffs, clusters, cluster_class, members), None where the call has none"""
    det, t = det or cfg.det, t or cfg.t
    if score == 0:
        return [(m, None, None, c, None, mem) for m, c, mem in det.collect_clusters(n, cap_total=1 << 17)]
    if score == 1:
        return [(m, d, None, c, None, mem) for m, d, c, mem in det.collect_clusters_depth(n, t, cap_total=1 << 17)]
    return [(m, d, nd, c, None, mem) for m, d, nd, c, mem in det.collect_clusters_depth_normal(n, t, cap_total=1 << 17)]


def same_frame(got, want, what):
    """one frame of ExportedClusters.to_host() against the same frame of a collect call, bit for bit; member ranges through each side's own
    flat member array (the two differ where an earlier frame was not delivered)"""
    assert got is not None, what
    for i, name in enumerate(("matches", "diffs", "ndiffs")):
        assert (got[i] is None) == (want[i] is None), (what, name)
        if want[i] is not None:
            assert got[i].tobytes() == np.ascontiguousarray(want[i]).tobytes(), (what, name)
    c, wc = got[3], want[3]
    assert len(c) == len(wc), (what, len(c), len(wc))
    for fld in ("index", "rect", "member_count"):
        assert np.array_equal(c[fld], wc[fld]), (what, fld)
    assert c["score"].tobytes() == wc["score"].tobytes(), (what, "score bits")
    assert (got[4] is None) == (want[4] is None) and (want[4] is None or np.array_equal(got[4], want[4])), (what, "cluster_class")
    for a, b in zip(c, wc):
        assert np.array_equal(got[5][a["member_begin"]:a["member_begin"] + a["member_count"]], want[5][b["member_begin"]:b["member_begin"] + b["member_count"]]), what


def same_batch(host, collected, what, whole=True):
    for f, (g, w) in enumerate(zip(host, collected)):
        same_frame(g, w, (what, f))
    if whole:                                                              # every frame delivered: the flat arrays are the collect's, member_begin included
        n_mem = sum(int(w[3]["member_count"].sum()) for w in collected)
        assert np.array_equal(host[0][5], collected[0][5][:n_mem]), what
        for g, w in zip(host, collected):
            assert np.array_equal(g[3]["member_begin"], w[3]["member_begin"]), what


def reference(cfg, names, score, alt=False):
    """what the collect call returns for this batch and scene, computed once per (batch, score, scene)"""
    key = (tuple(names), score, alt)
    if key not in cfg.cache:
        upload_enqueue(cfg, names)
        if score:
            cfg.t.upload_scene_device(scene_of(cfg, names, alt))
        cfg.cache[key] = collect(cfg, len(names), score)
    return cfg.cache[key]


def check_info(res, collected):
    """frame_info and header as include/lmx.h lays them out, from the collect's counts"""
    info, header = res.frame_info.cpu().numpy(), res.header.cpu().numpy()
    pos = [0, 0, 0]
    for f, w in enumerate(collected):
        nmem = int(w[3]["member_count"].sum())
        assert info[f, :7].tolist() == [pos[0], len(w[0]), pos[1], len(w[3]), pos[2], nmem, 0], (f, info[f])
        pos = [pos[0] + len(w[0]), pos[1] + len(w[3]), pos[2] + nmem]
    assert header[:5].tolist() == [len(collected), 0] + pos and header[6] == info[:, 7].sum() and not header[7:].any(), header
    return info


@pytest.mark.parametrize("score", SCORES)
def test_unclassed_chains_equal_their_collect(cfg, score):
    names = ["A", "Z", "B"]
    upload_enqueue(cfg, names)
    if score:
        cfg.t.upload_scene_device(scene_of(cfg, names))
    res = export(cfg, 3, score)
    assert res.header.is_cuda and (res.diffs is None) == (score == 0) and (res.ndiffs is None) == (score < 2) and res.cluster_class is None
    host = res.to_host()
    tensors = {k: v.clone() for k, v in res._backing.items()}
    if score == 0:                                                         # the same enqueue through the older entry point
        old = cfg.det.export_matches(3, clusters=True, max_large_frames=1)
        torch.cuda.synchronize()
        n_m, n_c, n_mem = (int(v) for v in old.header[2:5].cpu())
        assert torch.equal(old.header, res.header) and torch.equal(old.frame_info, res.frame_info)
        assert torch.equal(old.matches[:n_m], res.matches[:n_m]) and torch.equal(old.clusters[:n_c], res.clusters[:n_c]) and torch.equal(old.members[:n_mem], res.members[:n_mem])
    else:                                                                  # a one-class bank: class_index 0 selects every match
        again = export(cfg, 3, score, class_index=0)
        torch.cuda.synchronize()
        n_m, n_c = int(again.header[2]), int(again.header[3])
        assert torch.equal(again.frame_info, tensors["frame_info"]) and torch.equal(again.diffs[:n_m], tensors["diffs"][:n_m])
        assert torch.equal(again.clusters[:n_c], tensors["clusters"][:n_c])
    collected = collect(cfg, 3, score)                                     # the same enqueue, after the export
    info = check_info(res, collected)
    assert info[0, 7] > cc.F2_MAX and info[1, 7] == 0 and 0 < info[2, 7] < cc.F2_MAX, info[:, 7]        # the large-frame kernel, nothing, the LDS kernel
    assert len(collected[0][3]) > 0 and len(collected[2][3]) > 0
    same_batch(host, collected, ("A Z B", score))
    if score:
        assert (collected[0][1]["n_valid"] > 0).any()
        cfg.cache[(tuple(names), score, False)] = collected
    if score == 2:
        assert (collected[0][2]["n_normal"] >= 0).all()


def test_without_large_frames_a_is_handed_back_and_collect_finishes_it(cfg):
    names = ["A", "Z", "B"]
    want = reference(cfg, names, 1)
    upload_enqueue(cfg, names)
    cfg.t.upload_scene_device(scene_of(cfg, names))
    res = export(cfg, 3, 1, max_large_frames=0)
    host = res.to_host()
    info, header = res.frame_info.cpu().numpy(), res.header.cpu().numpy()
    assert host[0] is None and info[0].tolist() == [0, 0, 0, 0, 0, 0, 1, info[0, 7]] and info[0, 7] > cc.F2_MAX and header[1] == 2
    assert info[2, :7].tolist() == [0, len(want[2][0]), 0, len(want[2][3]), 0, int(want[2][3]["member_count"].sum()), 0]      # B starts at 0: A adds nothing
    same_frame(host[1], want[1], "Z")
    same_frame(host[2], want[2], "B")
    same_batch(collect(cfg, 3, 1), want, "collect after the export", whole=False)


# ---- 3. end to end, classes ----------------------------------------------------------------------------------------------------------------------
def classes_export(tc, n, mode, t, **kw):
    score = ("similarity", "depth", "normal").index(mode)
    return tc.det.export_clusters(n, templates=t if score else None, normals=score == 2, classes=True, class_base=class_base_of(tc.crops) if score else None,
                                  max_large_frames=1, **kw)


def classes_scene(tc, n):
    if not hasattr(tc, "dev_depth"):
        tc.dev_depth = [torch.from_numpy(d.view(np.int16)).cuda() for d in tc.depth]
    return tc.dev_depth[:n]


@pytest.mark.parametrize("mode", ("similarity", "depth", "normal"))
def test_classed_chains_equal_collect_clusters_classes(two_classes, mode):  # noqa: F811
    tc = two_classes
    t = joined_object(tc.crops, mode == "normal") if mode != "similarity" else None
    tc.det.upload(tc.frames)
    for n in (1, 3):
        tc.det.enqueue(n, E2E["threshold"])
        if t is not None:
            t.upload_scene_device(classes_scene(tc, n))
        res = classes_export(tc, n, mode, t)
        host = res.to_host()
        if t is None:
            want = tc.det.collect_clusters_classes(n)
        else:
            want = tc.det.collect_clusters_classes(n, t, class_base_of(tc.crops), normals=mode == "normal")
        check_info(res, want)
        same_batch(host, want, (mode, n))
        k = want[0][4]
        assert (k == 0).any() and (k == 1).any() and res.cluster_class is not None      # both classes have clusters
    if t is not None:
        t.close()


# ---- 4. capacities ---------------------------------------------------------------------------------------------------------------------------------
def test_side_arrays_follow_their_parents_fit(two_classes):  # noqa: F811
    tc = two_classes
    t = joined_object(tc.crops, True)
    tc.det.upload(tc.frames)
    tc.det.enqueue(3, E2E["threshold"])
    t.upload_scene_device(classes_scene(tc, 3))
    stream = torch.cuda.current_stream()
    full = classes_export(tc, 3, "normal", t)
    want = full.to_host()
    fi = full.frame_info.cpu().numpy()
    tm, tc_, tmem = (int(v) for v in full.header[2:5].cpu())
    assert fi[2, 1] > 0 and fi[2, 3] > 0                                    # the last frame has matches and clusters to lose

    def run(caps):
        buf = ExportedClusters(3, 2, True, (tm + 8, tc_ + 8, tmem + 8), stream, 0)
        for v in buf._backing.values():
            v.view(torch.uint8).fill_(CANARY)
        res = classes_export(tc, 3, "normal", t, cap_matches=caps[0], cap_clusters=caps[1], cap_members=caps[2], out=buf)
        assert res is buf
        stream.synchronize()
        hdr, info = res.header.cpu().numpy(), res.frame_info.cpu().numpy()
        assert hdr[2:5].tolist() == [tm, tc_, tmem]                          # the true totals, whatever fitted
        raw = {k: v.cpu().numpy().view(np.uint8).reshape(len(v), -1) for k, v in buf._backing.items()}
        for k, cap in (("matches", caps[0]), ("diffs", caps[0]), ("ndiffs", caps[0]), ("clusters", caps[1]), ("cluster_class", caps[1]), ("members", caps[2])):
            assert (raw[k][cap:] == CANARY).all(), k                          # nothing behind a capacity
        return hdr, info, raw, res.to_host()

    hdr, info, raw, host = run((tm, tc_, tmem))                              # exactly the totals: everything arrives
    assert hdr[1] == 0 and info[:, 6].tolist() == [0, 0, 0]
    for f in range(3):
        same_frame(host[f], want[f], ("exact", f))
    mb, cb = int(fi[2, 0]), int(fi[2, 2])
    hdr, info, raw, host = run((tm - 1, tc_, tmem))                          # one match short: the last frame's matches, diffs and ndiffs stay unwritten
    assert hdr[1] == 4 and info[:, 6].tolist() == [0, 0, 4] and host[2] is None
    for k in ("matches", "diffs", "ndiffs"):
        assert (raw[k][mb:] == CANARY).all(), k
    assert np.array_equal(raw["cluster_class"][cb:tc_].view(np.int32).reshape(-1), want[2][4])
    same_frame(host[1], want[1], "one match short, frame 1")
    hdr, info, raw, host = run((tm, tc_ - 1, tmem))                          # one cluster short: clusters, cluster_class and members stay unwritten
    assert hdr[1] == 4 and info[:, 6].tolist() == [0, 0, 8]
    for k, at in (("clusters", cb), ("cluster_class", cb), ("members", int(fi[2, 4]))):
        assert (raw[k][at:] == CANARY).all(), k
    assert raw["diffs"][mb:tm].tobytes() == want[2][1].tobytes() and raw["ndiffs"][mb:tm].tobytes() == want[2][2].tobytes()
    tc.det.release()
    t.close()


# ---- 5. ordering and lifetime ------------------------------------------------------------------------------------------------------------------
def test_the_next_scene_waits_for_the_export_on_the_device(cfg):
    names = ["A", "Z", "B"]
    want = [reference(cfg, names, 2), reference(cfg, names, 2, alt=True)]
    assert want[0][0][1].tobytes() != want[1][0][1].tobytes()                # the scenes differ where it counts
    s = torch.cuda.Stream()
    upload_enqueue(cfg, names, stream=s)
    cfg.t.upload_scene_device(scene_of(cfg, names), stream=s)
    first = export(cfg, 3, 2, stream=s)
    cfg.t.upload_scene_device(scene_of(cfg, names, alt=True), stream=s)     # at once: the copies wait for the walk on the device
    cfg.det.enqueue(3, THR)
    second = export(cfg, 3, 2, stream=s)
    same_batch(first.to_host(), want[0], "first scene")
    same_batch(second.to_host(), want[1], "second scene")
    cfg.det.release()
    cfg.det.release()


def filler_for(s, ms):
    """-> a function that queues about `ms` milliseconds of matrix products on stream s"""
    with torch.cuda.stream(s):
        a = torch.randn((2048, 2048), device="cuda")

    def filler(n):
        with torch.cuda.stream(s):
            for _ in range(n):
                torch.mm(a, a)

    n, t0, t1 = 16, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        t0.record(s)
        filler(n)
        t1.record(s)
        s.synchronize()
        if t0.elapsed_time(t1) >= ms:
            return lambda: filler(n)
        n *= 2
        assert n <= 1 << 16


def test_nothing_waits_and_close_waits_for_the_export(cfg):
    names = ["A", "Z", "B"]
    want = reference(cfg, names, 2)
    s = torch.cuda.Stream()
    t = DepthTemplates.from_crops(cfg.crops)
    t.enable_normals(FX, FY)

    def step():
        upload_enqueue(cfg, names, stream=s)
        t.upload_scene_device(scene_of(cfg, names), stream=s)
        return export(cfg, 3, 2, t=t, stream=s)

    res = step()                                                            # warm-up: buffers, the scene, the kernels' code
    s.synchronize()
    cfg.det.release()
    fill = filler_for(s, 50.0)
    fill()
    res = step()
    done = torch.cuda.Event()
    done.record(s)
    assert not done.query()                                                 # upload_device, enqueue, upload_scene_device and export_clusters returned with the filler still running
    t.close()                                                               # waits for the walk, which waits for the filler: the crops are not freed under it
    same_batch(res.to_host(), want, "closed directly after the export")
    cfg.det.release()


def test_three_enqueues_exported_oldest_first(cfg):
    batches = [["A", "Z", "B"], ["B", "Z", "B"], ["Z", "B", "A"]]
    want = [reference(cfg, names, 1) for names in batches]
    det = Detector(cfg.bank, S, S, max_batch=3, max_candidates=1 << 17, overlap=True)
    det.set_cluster_sidecar(cfg.dists, cfg.rects, *SIDE)
    s = torch.cuda.Stream()
    for names in batches:
        upload_enqueue(cfg, names, det=det, stream=s)
    kept, buf = [], None
    for names in batches:
        cfg.t.upload_scene_device(scene_of(cfg, names), stream=s)          # each export's scene, behind the export before it
        buf = export(cfg, 3, 1, det=det, oldest=True, stream=s, out=buf)   # one set of buffers, written three times
        kept.append(buf.clone())
        det.release()
    s.synchronize()
    for names, res, w in zip(batches, kept, want):
        same_batch(res.to_host(), w, names)
    det.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_enqueue_and_the_context_usable(cfg):
    det = Detector(cfg.bank, S, S, max_batch=2, max_candidates=1 << 17)
    L = _lib.lib()
    stream = torch.cuda.current_stream()
    buf = ExportedClusters(1, 2, True, (1 << 12, 256, 1 << 12), stream, 0)
    b = buf._backing
    t = DepthTemplates.from_crops(cfg.crops)
    base = np.asarray([0, N_T], np.int32)

    def desc(**kw):
        d = _lib.ExportClustersDesc(C.sizeof(_lib.ExportClustersDesc), 0, 1, 0, 1, -1, 0, 0, t.h, None, -np.inf, b["header"].data_ptr(), b["frame_info"].data_ptr(),
                                    b["matches"].data_ptr(), 1 << 12, b["diffs"].data_ptr(), b["ndiffs"].data_ptr(), b["clusters"].data_ptr(), 256,
                                    b["cluster_class"].data_ptr(), b["members"].data_ptr(), 1 << 12)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(word, n_frames=1, code=_lib.LMX_ERR_INVALID_ARG, **kw):
        d = desc(**kw)
        st = L.lmx_ctx_export_clusters_on(det.h, n_frames, C.byref(d), int(stream.cuda_stream))
        assert st == code, (word, st, L.lmx_last_error().decode())
        assert word in L.lmx_last_error().decode(), (word, L.lmx_last_error().decode())

    det.set_cluster_sidecar(cfg.dists, cfg.rects, *SIDE)
    refused("nothing enqueued")
    det.upload_device([cfg.dev["B"]])
    det.enqueue(1, THR)
    refused("struct_size", struct_size=C.sizeof(_lib.ExportClustersDesc) - 8)
    refused("struct_size", struct_size=C.sizeof(_lib.ExportDesc))
    refused("n_frames", n_frames=2)
    refused("score", score=3)
    refused("classes", classes=2)
    for name in ("header", "frame_info", "matches"):
        refused("must not be null", **{name: None})
    refused("clusters_out", clusters_out=None)
    refused("members", members=None)
    refused("templates and diffs", templates=None)
    refused("templates and diffs", diffs=None)
    refused("ndiffs", score=2, ndiffs=None)
    refused("lmx_ctx_set_cluster_sidecar_class", classes=1, score=0)           # no per-class side-car
    refused("max_large_frames", max_large_frames=-1)
    refused("not a number", no_value=float("nan"))
    refused("no scene uploaded")                                               # the collect path's conditions, through the same code
    t.upload_scene_device([cfg.scene["B"], cfg.scene["B"]])
    refused("scene holds 2 frames")
    t.upload_scene_device([cfg.scene["B"][:96, :80].contiguous()])
    refused("uploaded scene is 80 x 96")
    t.upload_scene_device([cfg.scene["B"]])
    refused("enable_normals", score=2)
    short = DepthTemplates.from_crops(cfg.crops[:5])
    short.upload_scene_device([cfg.scene["B"]])
    refused("5 depth templates", templates=short.h)
    short.close()
    # the per-class conditions
    det.set_cluster_sidecar_class(0, cfg.dists, cfg.rects, *SIDE)
    refused("cluster_class must not be null", classes=1, score=0, cluster_class=None)
    refused("class_base must hold", classes=1)
    wrong = np.asarray([0, N_T - 1], np.int32)
    refused("class_base gives it", classes=1, n_classes=1, class_base=wrong.ctypes.data)
    # outputs that are not plain device memory of the device, or misaligned
    host = np.zeros(1 << 12, DEPTH_DIFF_DTYPE)
    refused("diffs is", diffs=host.ctypes.data)
    arena = PinnedArena(1 << 16)
    pinned = arena.put(np.zeros(4096, np.int32))
    refused("cluster_class is", classes=1, n_classes=1, class_base=base.ctypes.data, cluster_class=pinned.ctypes.data)
    refused("diffs must be aligned to 8", diffs=b["diffs"].data_ptr() + 4)
    t.enable_normals(FX, FY)
    refused("ndiffs must be aligned to 8", score=2, ndiffs=b["ndiffs"].data_ptr() + 4)
    refused("cluster_class must be aligned", classes=1, n_classes=1, class_base=base.ctypes.data, cluster_class=b["cluster_class"].data_ptr() + 2)
    refused("clusters_out must be aligned", clusters_out=b["clusters"].data_ptr() + 4)
    # the enqueue is still there, and whole: the classed normal-scored export of a one-class bank, then the un-classed collect
    res = det.export_clusters(1, templates=t, normals=True, classes=True, class_base=base, max_large_frames=1, out=buf)
    host = res.to_host()[0]
    got = det.collect_clusters_depth_normal(1, t)[0]
    same_frame(host[:4] + (None,) + host[5:], (got[0], got[1], got[2], got[3], None, got[4]), "after the refusals")
    assert (host[4] == 0).all() and len(host[4]) == len(got[3]) > 0
    del arena
    t.close()
    det.close()
