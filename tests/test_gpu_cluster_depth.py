"""Depth-scored clusters on the device (lmx_ctx_collect_clusters_depth: the record form of k_walk, csrc/lmx_verify.hip, then the SCORED form of
k_f2_finalize_cluster, csrc/lmx_f2.hip) against the three-call composition it replaces: lmx_ctx_collect + lmx_depth_diff_matches +
lmx_cluster_matches_scored.  The expected values come from pieces the scored chain does not touch: cluster_cases.reference (numpy + the
real std::sort) for the final matches and the status, depth_verify_cases.np_diff for every match's difference, depth_values and the host
chain lmx_cluster_matches_scored on those.  Everything is compared with array_equal; nothing here has a tolerance."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import cluster_cases as cc
import depth_verify_cases as dvc
import mesh_cases as mc
from conftest import ROOT
from linemod_pose_estimation_amd import (DEPTH_DIFF_DTYPE, MATCH_DTYPE, DepthTemplates, Detector, NativeBank, _lib, cluster_matches_scored, depth_values,
                                         meshsynth as ms, synth)
from linemod_pose_estimation_amd.detector import debug_device_finalize_cluster_depth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

SCENE_W, SCENE_H = 96, 80


# ---- crops, scenes, the expected value --------------------------------------------------------------------------------------------------------

def make_crops(n, seed):
    """One crop per side-car template: widths across 8, 64 and 128 (dvc.WIDTHS), a few rows, zero holes; every seventh empty (not the first)."""
    rng = np.random.default_rng(seed)
    crops = []
    for k in range(n):
        if k % 7 == 5:
            crops.append(np.zeros((0, 0), np.uint16))
            continue
        w, h = dvc.WIDTHS[(5 * k + 1) % len(dvc.WIDTHS)], dvc.HEIGHTS[k % len(dvc.HEIGHTS)]
        crops.append(dvc._values(rng, (h, w), 0.3))
    return crops


def make_scenes(n, seed, zero=False):
    rng = np.random.default_rng(seed)
    return [np.zeros((SCENE_H, SCENE_W), np.uint16) if zero else dvc._values(rng, (SCENE_H, SCENE_W), 0.2) for _ in range(n)]


def values_of(diffs, no_value):
    v = depth_values(diffs)
    v[diffs["n_valid"] <= 0] = no_value
    return v


def np_diffs(matches, crops, scene, class_index=-1):
    """DEPTH_DIFF_DTYPE per match from the numpy restatement; zeros for another class and for a template the crops do not hold."""
    out = np.zeros(len(matches), DEPTH_DIFF_DTYPE)
    seen = {}
    for i, m in enumerate(matches):
        t = int(m["template_id"])
        if (class_index >= 0 and int(m["class_index"]) != class_index) or t < 0 or t >= len(crops):
            continue
        key = (t, int(m["x"]), int(m["y"]))
        if key not in seen:
            seen[key] = dvc.np_diff(crops[t], scene, key[1], key[2]) if crops[t].size else (0, 0, 0)
        out[i] = seen[key]
    return out


def expected(case, crops, scenes, class_index=-1, no_value=-np.inf):
    """Per frame: namespace(status, n_records, matches, diffs, clusters, members); clusters None where the device reports none."""
    out = []
    for f, r in enumerate(cc.reference(case)):
        e = SimpleNamespace(status=r.status, n_records=r.n_records, matches=r.matches, diffs=None, clusters=None, members=None)
        if r.status != 1:
            e.diffs = np_diffs(r.matches, crops, scenes[f], class_index)
        if r.status == 0:
            m = np.ascontiguousarray(r.matches).astype(MATCH_DTYPE)
            c, mem = cluster_matches_scored(m, values_of(e.diffs, no_value), case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)
            e.clusters, e.members = c, mem[:int(c["member_count"].sum()) if len(c) else 0].copy()
        out.append(e)
    return out


def check_case(case, crops, scenes, class_index=-1, no_value=-np.inf, want=None, templates=None):
    want = expected(case, crops, scenes, class_index, no_value) if want is None else want
    t = templates if templates is not None else DepthTemplates.from_crops(crops)
    try:
        got, counts = debug_device_finalize_cluster_depth(case.records, case.n_frames, t, scenes, case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh,
                                                          class_index=class_index, no_value=no_value, with_counts=True)
    finally:
        if templates is None:
            t.close()
    assert len(got) == case.n_frames
    for f in range(case.n_frames):
        what = (case.name, f)
        m, d, c, mem, status = got[f]
        e = want[f]
        assert status == e.status, (what, status, e.status, counts[f].tolist())
        if status == 1:       # too many records: the count, nothing else
            assert counts[f].tolist() == [e.n_records, 0, 0, 1], what
            continue
        assert counts[f][0] == len(e.matches), (what, counts[f].tolist(), len(e.matches))
        for k in cc.FIELDS:
            assert np.array_equal(m[k], e.matches[k]), (what, k)
        for k in DEPTH_DIFF_DTYPE.names:
            assert np.array_equal(d[k], e.diffs[k]), (what, k)
        if status == 2:       # side-car / range: the final matches and their diffs, no clusters
            assert counts[f].tolist() == [len(e.matches), 0, 0, 2], what
            continue
        assert counts[f].tolist() == [len(e.matches), len(e.clusters), len(e.members), 0], (what, counts[f].tolist())
        for k in cc.CLUSTER_FIELDS:
            assert np.array_equal(c[k], e.clusters[k]), (what, k)
        assert c["score"].tobytes() == e.clusters["score"].tobytes(), (what, "score bits")
        assert np.array_equal(mem, e.members), (what, "members")
    return want


# ---- 1. the constructed cases ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_constructed_case_with_the_depth_score(name):
    case = cc.case_by_name(name)
    crops, scenes = make_crops(len(case.dists), 500 + cc.CASE_NAMES.index(name)), make_scenes(case.n_frames, 600 + cc.CASE_NAMES.index(name))
    want = expected(case, crops, scenes)
    ref = cc.reference(case)
    if name == "origin":      # matches left of and above the image: crops partly outside it, some still counting
        m, d = want[0].matches, want[0].diffs
        cut = (m["x"] < 0) | (m["y"] < 0)
        assert cut.any() and (d["n_valid"][cut] <= d["n_template"][cut]).all() and ((d["n_valid"][cut] > 0) & (d["n_valid"][cut] < d["n_template"][cut])).any()
    if name == "score_ties":  # the depth score orders the same clusters differently than the mean similarity: the two instantiations differ
        by_sim, by_depth = [tuple(i) for i in ref[2].clusters["index"]], [tuple(i) for i in want[2].clusters["index"]]
        assert sorted(by_sim) == sorted(by_depth) and len(by_sim) == 40 and by_sim != by_depth
        score = want[2].clusters["score"]
        assert np.isfinite(score).sum() >= 3 and np.array_equal(score, np.sort(score)[::-1])
    check_case(case, crops, scenes, want=want)


# ---- 2. the duplicate that decides ----------------------------------------------------------------------------------------------------------------

def test_the_surviving_duplicate_brings_its_own_diff():
    """Two records equal in (x, y, similarity, class) with templates 1 and 3: std::unique keeps the one the sort put first (template 1), and
    the surviving match carries template 1's difference, whichever of the two arrived first."""
    rng = np.random.default_rng(71)
    crops = [dvc._values(rng, (h, w), 0.0) for (w, h) in ((9, 4), (20, 5), (7, 3), (33, 9))]
    scenes = make_scenes(1, 72)
    dists, rects = np.full(4, 0.72), np.asarray([[0, 0, c.shape[1], c.shape[0]] for c in crops], np.int32)
    s = 88.5
    rows = np.array([(30, 40, s, 1, 0), (30, 40, s, 3, 0), (10, 10, 70.0, 0, 0), (60, 20, 60.0, 2, 0)], np.float64)
    rec = cc.frame_records(rng, 0, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4])
    case = cc.Case("depth_duplicate", rec, 1, dists, rects, 10, thresh=0)
    want = expected(case, crops, scenes)
    m, d = want[0].matches, want[0].diffs
    assert len(m) == 3 and m["template_id"].tolist() == [1, 0, 2]
    survivor, loser = dvc.np_diff(crops[1], scenes[0], 30, 40), dvc.np_diff(crops[3], scenes[0], 30, 40)
    assert survivor != loser and survivor[1] > 0 and loser[1] > 0
    assert (int(d["sum_abs_mm"][0]), int(d["n_valid"][0]), int(d["n_template"][0])) == survivor
    orders = set()
    for variant in (case, cc.shuffled(case, 1), cc.shuffled(case, 2), cc.shuffled(case, 3), cc.shuffled(case, 4)):
        t = variant.records["template_id"].tolist()
        orders.add(t.index(1) < t.index(3))
        check_case(variant, crops, scenes, want=want)
    assert orders == {True, False}       # both arrival orders were run


# ---- 3. score ties under the depth score -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("no_value", [-np.inf, -1.5])
def test_all_clusters_tie_at_no_value(no_value):
    """An all-zero scene: n_valid == 0 everywhere, every cluster scores no_value, the order is std::sort's order of ties (16, 17 and 40
    clusters: insertion sort below 17, introsort above)."""
    case = cc.case_by_name("score_ties")
    crops, scenes = make_crops(len(case.dists), 81), make_scenes(case.n_frames, 82, zero=True)
    want = expected(case, crops, scenes, no_value=no_value)
    for e in want:
        assert not e.diffs["n_valid"].any() and e.diffs["n_template"].any() and len(e.clusters) >= 16 and (e.clusters["score"] == no_value).all()
    check_case(case, crops, scenes, no_value=no_value, want=want)


# ---- 4. record counts and frames --------------------------------------------------------------------------------------------------------------

def _lattice_case(name, sizes, seed, n_t=9, extra=()):
    rng = np.random.default_rng(seed)
    dists, rects = cc.sidecar(rng, n_t)
    parts = [cc.draw_frame(rng, f, n, n_t, cc.SIMS[:3], grid=(4, 3), pitch=20) for f, n in enumerate(sizes)] + list(extra)
    return cc.Case(name, cc.interleave(rng, parts), len(sizes), dists, rects, 10, thresh=1)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_record_counts_around_the_workgroup_size(n):
    case = _lattice_case("depth_count%d" % n, [n], 900 + n)
    crops, scenes = make_crops(9, 91), make_scenes(1, 92)
    want = check_case(case, crops, scenes)
    assert want[0].n_records == n and want[0].status == 0 and (n < 255 or (len(want[0].clusters) > 2 and (want[0].diffs["n_valid"] > 0).any()))


def test_2048_records_run_and_2049_are_handed_back():
    case = _lattice_case("depth_full", [2048, 2049], 93)
    crops, scenes = make_crops(9, 94), make_scenes(2, 95)
    want = check_case(case, crops, scenes)
    assert [e.n_records for e in want] == [2048, 2049] and [e.status for e in want] == [0, 1] and len(want[0].clusters) > 2


def test_eight_frames_interleaved_stray_frames_and_a_template_outside_the_table():
    rng = np.random.default_rng(96)
    stray = [cc.draw_frame(rng, -1, 30, 9, cc.SIMS[:3], grid=(4, 3)), cc.draw_frame(rng, 8, 30, 9, cc.SIMS[:3], grid=(4, 3)),
             cc.draw_frame(rng, 1000, 5, 9, cc.SIMS[:3], grid=(4, 3))]
    bad = cc.frame_records(rng, 5, [33], [21], [99.0], [9])          # template id == count == the side-car's size, the frame's best match
    case = _lattice_case("depth_eight", [60, 0, 130, 7, 300, 41, 1, 90], 97, extra=stray + [bad])
    crops = make_crops(9, 98)
    scenes = make_scenes(8, 99)
    assert any(not np.array_equal(scenes[0], s) for s in scenes[1:])
    want = check_case(case, crops, scenes)
    assert [e.status for e in want] == [0, 0, 0, 0, 0, 2, 0, 0] and [e.n_records for e in want] == [60, 0, 130, 7, 300, 42, 1, 90]
    e = want[5]
    assert e.matches["template_id"][0] == 9 and not any(e.diffs[k][0] for k in DEPTH_DIFF_DTYPE.names) and (e.diffs["n_template"][1:] > 0).any()
    # the frame index reaches the kernel: the same matches against another frame's scene give other numbers
    assert not np.array_equal(np_diffs(want[4].matches, crops, scenes[0])["sum_abs_mm"], want[4].diffs["sum_abs_mm"])


# ---- 5. class_index ---------------------------------------------------------------------------------------------------------------------------

def test_class_filter_gives_the_other_class_zero_diffs_and_no_value():
    case = _lattice_case("depth_classes", [400, 90], 101)       # draw_frame: two classes
    crops, scenes = make_crops(9, 102), make_scenes(2, 103)
    free = expected(case, crops, scenes)
    for no_value in (-np.inf, -0.25):
        want = expected(case, crops, scenes, class_index=1, no_value=no_value)
        m, d = want[0].matches, want[0].diffs
        other = m["class_index"] != 1
        assert other.any() and (~other).any() and not d["n_template"][other].any() and d["n_template"][~other].any()
        assert free[0].diffs["n_template"][other].any()
        assert any(not np.array_equal(want[0].clusters[k], free[0].clusters[k]) for k in ("index", "score"))
        check_case(case, crops, scenes, class_index=1, no_value=no_value, want=want)


# ---- 6. seeded random draws ---------------------------------------------------------------------------------------------------------------------

def test_random_draws_with_the_depth_score():
    scenes = make_scenes(4, 111)
    for seed in range(40):
        case = cc.random_case(seed)
        crops = make_crops(len(case.dists), 2000 + seed)
        check_case(case, crops, scenes[:case.n_frames])


# ---- 7. end to end at 320 x 240 -------------------------------------------------------------------------------------------------------------------

F = ms.ENSENSO["fx"]
W, H = 320, 240
THRESHOLD = 75.0


def assert_frame_equals_composition(got, matches, diffs, clusters, members, what):
    m, d, c, mem = got
    assert len(m) == len(matches), (what, len(m), len(matches))
    for k in cc.FIELDS:
        assert np.array_equal(m[k], matches[k]), (what, k)
    assert d.tobytes() == diffs.tobytes(), what
    assert len(c) == len(clusters), (what, len(c), len(clusters))
    for k in ("index", "rect", "member_count"):
        assert np.array_equal(c[k], clusters[k]), (what, k)
    assert c["score"].tobytes() == clusters["score"].tobytes(), what
    for a, b in zip(c, clusters):
        assert np.array_equal(mem[a["member_begin"]:a["member_begin"] + a["member_count"]], members[b["member_begin"]:b["member_begin"] + b["member_count"]]), what


@pytest.fixture(scope="module")
def trained():
    """The bank and scene of test_gpu_depth_verify.py's `trained` fixture (204 views of the chip at 320 x 240, two instances), a second scene,
    the templates' depth renders and a context with the side-car."""
    chip, cpu = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary")
    views = ms.view_grid()[:204]
    b = ms.empty_bank()
    nb = NativeBank.create(b.T, b.modalities)
    nb.train_mesh(chip, views, W, H, F / 2, F / 2)
    sc = nb.last_side_car
    frames = [ms.make_scene(chip, views, width=W, height=H, seed=seed, n_instances=2, fx=F / 2, fy=F / 2, other_tri=cpu, n_other=1, margin=44)[0] for seed in (11, 12)]
    det = Detector(nb, W, H, max_batch=2)
    det.set_cluster_sidecar(sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
    t = DepthTemplates.from_mesh(chip, list(zip(sc["R"], sc["T"][:, 2])), W, H, F / 2, F / 2)
    yield SimpleNamespace(chip=chip, views=views, sc=sc, frames=frames, det=det, t=t)
    t.close()
    det.close()


def composition(tr, per_frame, depth, class_index=-1, no_value=-np.inf):
    """collect's matches through DepthTemplates.diff + cluster_matches_scored -> per frame (matches, diffs, clusters, members)."""
    flat = np.concatenate(per_frame)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in per_frame])])
    diffs = tr.t.diff(depth, flat, offsets, class_index=class_index)
    out = []
    for f in range(len(per_frame)):
        d = diffs[offsets[f]:offsets[f + 1]]
        c, mem = cluster_matches_scored(per_frame[f], values_of(d, no_value), tr.sc["obj_origin_dists"], tr.sc["rects"], 10, 0.4, 0.05, 2)
        out.append((per_frame[f], d, c, mem))
    return out


def test_end_to_end_equals_the_composition(trained):
    tr = trained
    tr.det.upload(tr.frames)
    tr.det.enqueue(2, THRESHOLD)
    tr.det.enqueue(2, THRESHOLD)
    want = composition(tr, tr.det.collect(2), [fr[1] for fr in tr.frames])
    tr.t.upload_scene([fr[1] for fr in tr.frames])
    got = tr.det.collect_clusters_depth(2, tr.t)
    for f in range(2):
        assert_frame_equals_composition(got[f], *want[f], what=f)
    m, d, c, _ = want[0]          # the scene of test_gpu_depth_verify.py: a few hundred matches, every one with something to compare
    assert 100 < len(m) < 2000 and len(c) >= 1 and np.isfinite(c["score"]).all() and (c["score"] < 0).all() and (d["n_valid"] > 0).all()
    assert len(want[1][0]) > 0 and want[0][1].tobytes() != want[1][1].tobytes()


# ---- 8. host fallback end to end ------------------------------------------------------------------------------------------------------------------

def test_a_frame_beyond_2048_records_is_finished_on_the_host_with_the_depth_score():
    """The configuration of test_gpu_cluster_chain.py's fallback test: frame 0 leaves more than 2048 raw records (asserted on the oracle's
    count) and is finished on the host inside the call, frame 1 takes the device chain; both equal the composition."""
    S = 160
    thr, n_t = 45.0, 80
    bank = synth.make_bank(n_t, seed=91, size_range=(20.0, 36.0))
    frames = [synth.make_scene(bank, S, S, seed=94)[0], synth.make_scene(bank, S, S, seed=93, n_instances=1)[0]]
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(n_t) % 4) + rng.uniform(-0.005, 0.005, n_t)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    crops = [dvc._values(rng, (int(r[3]), int(r[2])), 0.3) for r in rects]
    depth = [np.ascontiguousarray(fr[1]) for fr in frames]
    assert all((d != 0).any() for d in depth)
    od = o.OracleDetector(bank)
    sizes = []
    for f in range(2):
        od.match(frames[f], thr)
        sizes.append(len(od.last_raw()))
    assert sizes[0] > cc.F2_MAX > sizes[1] > 0, sizes
    t = DepthTemplates.from_crops(crops)
    det = Detector(bank, S, S, max_batch=2, max_candidates=1 << 17)
    det.set_cluster_sidecar(dists, rects, 10, 0.5, 0.1, 2)
    det.upload(frames)
    det.enqueue(2, thr)
    det.enqueue(2, thr)
    per_frame = det.collect(2, cap_total=1 << 17)
    t.upload_scene(depth)
    got = det.collect_clusters_depth(2, t, cap_total=1 << 17)
    for f in range(2):
        d = t.diff(depth[f], per_frame[f])
        want_d = np_diffs(per_frame[f], crops, depth[f])
        assert d.tobytes() == want_d.tobytes() and (d["n_valid"] > 0).any()
        c, mem = cluster_matches_scored(per_frame[f], depth_values(d), dists, rects, 10, 0.5, 0.1, 2)
        assert len(c) > 0
        assert_frame_equals_composition(got[f], per_frame[f], d, c, mem, what=f)
    t.close()
    det.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_enqueue_outstanding(trained):
    tr = trained
    depth = [fr[1] for fr in tr.frames]
    few = DepthTemplates.from_crops([np.ones((3, 3), np.uint16)] * 5)
    fresh = DepthTemplates.from_crops([np.ones((3, 3), np.uint16)] * len(tr.sc["rects"]))

    def refused(templates, n_frames=2, no_value=-np.inf):
        with pytest.raises(_lib.LmxError) as e:
            tr.det.collect_clusters_depth(n_frames, templates, no_value=no_value)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG
        return str(e.value)

    tr.det.upload(tr.frames)
    tr.det.enqueue(2, THRESHOLD)
    assert "no scene uploaded" in refused(fresh)
    tr.t.diff(depth[0], np.zeros(1, MATCH_DTYPE))           # the host-list call forgets an uploaded scene
    tr.t.upload_scene(depth)
    tr.t.diff(depth[0], np.zeros(1, MATCH_DTYPE))
    assert "no scene uploaded" in refused(tr.t)
    tr.t.upload_scene(depth[:1])
    assert "holds 1 frames" in refused(tr.t)
    tr.t.upload_scene([np.ascontiguousarray(d[:, :W - 8]) for d in depth])
    assert "%d x %d" % (W - 8, H) in refused(tr.t)
    few.upload_scene(depth)
    assert "5 depth templates" in refused(few)
    tr.t.upload_scene(depth)
    assert "not a number" in refused(tr.t, no_value=float("nan"))
    assert "n_frames=1" in refused(tr.t, n_frames=1)
    got = tr.det.collect_clusters_depth(2, tr.t)          # the enqueue is still there
    assert len(got) == 2 and len(got[0][0]) > 100 and len(got[0][2]) >= 1
    with pytest.raises(_lib.LmxError):                     # and now it is gone
        tr.det.collect_clusters_depth(2, tr.t)
    bare = Detector(tr.det.native_bank, W, H, max_batch=2)  # no side-car
    bare.upload(tr.frames)
    bare.enqueue(2, THRESHOLD)
    with pytest.raises(_lib.LmxError) as e:
        bare.collect_clusters_depth(2, tr.t)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "sidecar" in str(e.value)
    assert len(bare.collect(2)) == 2
    bare.close()
    few.close()
    fresh.close()


# ---- 10. two calls in a row -------------------------------------------------------------------------------------------------------------------

def test_a_second_scene_replaces_the_first(trained):
    tr = trained
    depth = [fr[1] for fr in tr.frames]
    further = [np.where(d != 0, d + 9, 0).astype(np.uint16) for d in depth]
    tr.det.upload(tr.frames)
    tr.det.enqueue(2, THRESHOLD)
    tr.det.enqueue(2, THRESHOLD)
    per_frame = tr.det.collect(2)
    want_a, want_b = composition(tr, per_frame, depth), composition(tr, per_frame, further)      # the same matches against either scene
    tr.t.upload_scene(depth)
    got_a = tr.det.collect_clusters_depth(2, tr.t)
    tr.det.enqueue(2, THRESHOLD)
    tr.t.upload_scene(further)                # nothing in flight: the staging buffer and the event are reused
    got_b = tr.det.collect_clusters_depth(2, tr.t)
    for f in range(2):
        assert_frame_equals_composition(got_a[f], *want_a[f], what=("first", f))
        assert_frame_equals_composition(got_b[f], *want_b[f], what=("second", f))
    assert want_a[0][1].tobytes() != want_b[0][1].tobytes() and want_a[0][2]["score"].tobytes() != want_b[0][2]["score"].tobytes()


# ---- 11. the C++ caller ---------------------------------------------------------------------------------------------------------------------------

def test_cpp_caller_prints_what_the_python_path_computes(trained, tmp_path):
    tr = trained
    exe = str(tmp_path / "cluster_depth_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cluster_depth_main.cpp"),
                           "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    sources = tr.frames[0]
    np.ascontiguousarray(tr.chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(tr.views).tofile(tmp_path / "views.f64")
    np.ascontiguousarray(sources[0]).tofile(tmp_path / "bgr.u8")
    np.ascontiguousarray(sources[1]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(W), str(H), repr(F / 2), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(THRESHOLD)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    tr.det.upload([sources])
    tr.det.enqueue(1, THRESHOLD)
    tr.t.upload_scene(sources[1])
    m, d, clusters, _ = tr.det.collect_clusters_depth(1, tr.t)[0]
    want = ["templates %d depth_templates %d device_bytes %d" % (len(tr.sc["rects"]), len(tr.t), tr.t.device_bytes),
            "matches %d sum_abs_mm %d n_valid %d" % (len(m), d["sum_abs_mm"].sum(), d["n_valid"].sum())]
    want += ["cluster %d %d %d rect %d %d %d %d members %d mean_depth_difference_mm %.17g" % (tuple(c["index"]) + tuple(c["rect"]) + (c["member_count"], -1000.0 * c["score"]))
             for c in clusters]
    assert len(clusters) >= 1 and res.stdout.strip().splitlines() == want
