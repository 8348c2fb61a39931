"""The per-class consumer chain on the device: the CLASSES forms of k_f2_finalize_cluster through lmx_debug_device_finalize_cluster_classes
on the constructed cases of tests/cluster_class_cases.py (mean similarity, depth score, depth + normal score; three arrival orders),
lmx_depth_templates_append, and lmx_ctx_collect_clusters_classes end to end.  Two yardsticks, both independent of the new code: the
oracle's restatement applied per class (cluster_class_cases.reference), and the composition of entry points that existed before --
lmx_ctx_collect, per class a DepthTemplates of its own with diff / normal_diff at class_index = c, per class lmx_cluster_matches_scored.
Everything is compared bit for bit; nothing here has a tolerance."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import cluster_cases as cc
import cluster_class_cases as ccc
import golden_util
from conftest import ROOT
from linemod_pose_estimation_amd import (DEPTH_DIFF_DTYPE, MATCH_DTYPE, NORMAL_DIFF_DTYPE, DepthTemplates, Detector, _lib, cluster_matches_scored, depth_values,
                                         normal_values, synth)
from linemod_pose_estimation_amd.detector import cluster_matches, debug_device_finalize_cluster, debug_device_finalize_cluster_classes
from oracle import oracle as o

pytestmark = pytest.mark.gpu

MODES = ("similarity", "depth", "normal")
FX = FY = 520.0
ALL_CASES = ccc.CASE_NAMES + ("scored",)


def get_case(name):
    return ccc.scored_case() if name == "scored" else ccc.case_by_name(name)


# ---- crops, scenes, the expected values -----------------------------------------------------------------------------------------------------
def ramp(shape, base):
    """A tilted plane (2 mm per pixel in x, 3 in y): smooth enough for DepthNormal's taps at +-5 to count, so that a crop or scene of more
    than 11 x 11 pixels has valid normals."""
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (base + 2 * x + 3 * y).astype(np.uint16)


def crops_of(case):
    """Per class index: None (no side-car) or one crop per template of the side-car; the scored case brings its own."""
    if hasattr(case, "crops"):
        return case.crops
    rng = np.random.default_rng(900 + len(case.name))
    shapes = ((2, 3), (5, 9), (1, 1), (13, 15))
    return [None if s is None else [ramp(shapes[(t + c) % 4], int(rng.integers(600, 900))) for t in range(len(s.dists))] for c, s in enumerate(case.classes)]


def scenes_of(case):
    if hasattr(case, "scenes"):
        return case.scenes
    scenes = [ramp((ccc.SCENE_H, ccc.SCENE_W), 700 + 7 * f) for f in range(case.n_frames)]
    for f, s in enumerate(scenes):
        s[5 + f:9 + f, 20:26] = 0                                  # a hole
    return scenes


def class_base_of(crops):
    return np.concatenate([[0], np.cumsum([0 if c is None else len(c) for c in crops])]).astype(np.int32)


def joined_object(crops, normals):
    """The classes' objects appended in class order, as a caller builds the object of the classed calls."""
    t = DepthTemplates.from_crops([])
    for c in crops:
        if c:
            part = DepthTemplates.from_crops(c)
            t.append(part)
            assert len(part) == 0
            part.close()
    if normals:
        t.enable_normals(FX, FY)
    return t


def values_of(dd, nd, no_value):
    if nd is None:
        v = depth_values(dd)
        v[dd["n_valid"] <= 0] = no_value
    else:
        v = normal_values(dd, nd)
        v[(dd["n_valid"] <= 0) | (nd["n_normal"] <= 0)] = no_value
    return v


def per_class_diffs(crops, scenes, per_frame, normals):
    """Every class's matches against an object that holds that class's crops alone, through the un-classed entry points at class_index = c
    -> per frame (depth diffs, normal diffs or None)."""
    flat = np.ascontiguousarray(np.concatenate(per_frame)).astype(MATCH_DTYPE)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in per_frame])])
    dd, nd = np.zeros(len(flat), DEPTH_DIFF_DTYPE), np.zeros(len(flat), NORMAL_DIFF_DTYPE)
    for c, cr in enumerate(crops):
        if not cr:
            continue
        t = DepthTemplates.from_crops(cr)
        sel = flat["class_index"] == c
        # a template id the class's object does not hold has zero diffs by definition; the host-list calls refuse it, so it is kept from them
        asked = flat.copy()
        asked["class_index"][sel & ((flat["template_id"] < 0) | (flat["template_id"] >= len(cr)))] = -1
        if normals:
            t.enable_normals(FX, FY)
            a, b = t.normal_diff(scenes, asked, offsets, class_index=c)
            nd[sel] = b[sel]
        else:
            a = t.diff(scenes, asked, offsets, class_index=c)
        assert not a[~sel]["n_template"].any()
        dd[sel] = a[sel]
        t.close()
    return [(dd[offsets[f]:offsets[f + 1]], nd[offsets[f]:offsets[f + 1]] if normals else None) for f in range(len(per_frame))]


def composition(classes, m, values):
    """Per class lmx_cluster_matches (values None) or lmx_cluster_matches_scored, joined as include/lmx.h defines it."""
    def chain(c, s, mc, pos):
        mc = np.ascontiguousarray(mc).astype(MATCH_DTYPE)
        if values is None:
            return cluster_matches(mc, s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh)
        return cluster_matches_scored(mc, values[pos], s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh)
    return ccc.compose(m, classes, chain)


_EXPECTED = {}


def expected(case, mode, no_value=-np.inf):
    """Per frame namespace(status, n_records, matches, dd, nd, clusters, cluster_class, members), computed once per (case, mode)."""
    key = (case.name, mode, no_value)
    if key in _EXPECTED:
        return _EXPECTED[key]
    ref = ccc.reference(case)
    diffs = None
    if mode != "similarity":
        diffs = per_class_diffs(crops_of(case), scenes_of(case), [r.matches for r in ref], mode == "normal")
    out = []
    for f, r in enumerate(ref):
        e = SimpleNamespace(status=r.status, n_records=r.n_records, matches=r.matches, dd=None, nd=None, clusters=None, cluster_class=None, members=None)
        if diffs is not None:
            e.dd, e.nd = diffs[f]
        if r.status == 0:
            if mode == "similarity":      # the oracle's restatement per class, and the library's un-classed chain per class agrees with it
                e.clusters, e.cluster_class, e.members = r.clusters, r.cluster_class, r.members
                c2, k2, m2 = composition(case.classes, r.matches, None)
                assert np.array_equal(c2, r.clusters) and np.array_equal(k2, r.cluster_class) and np.array_equal(m2, r.members)
            else:
                e.clusters, e.cluster_class, e.members = composition(case.classes, r.matches, values_of(e.dd, e.nd, no_value))
        out.append(e)
    _EXPECTED[key] = out
    return out


def run_hook(case, mode, no_value=-np.inf, templates=None):
    if mode == "similarity":
        return debug_device_finalize_cluster_classes(case.records, case.n_frames, ccc.as_tuples(case), with_counts=True)
    crops = crops_of(case)
    t = templates if templates is not None else joined_object(crops, mode == "normal")
    try:
        return debug_device_finalize_cluster_classes(case.records, case.n_frames, ccc.as_tuples(case), t, class_base_of(crops), scenes_of(case), normals=mode == "normal",
                                                     no_value=no_value, with_counts=True)
    finally:
        if templates is None:
            t.close()


def check_hook(case, mode, want, no_value=-np.inf, templates=None):
    got, counts = run_hook(case, mode, no_value, templates)
    assert len(got) == case.n_frames
    for f in range(case.n_frames):
        what = (case.name, mode, f)
        m, dd, nd, c, k, mem, status = got[f]
        e = want[f]
        assert status == e.status, (what, status, e.status, counts[f].tolist())
        if status == 1:       # too many records: the count, nothing else
            assert counts[f].tolist() == [e.n_records, 0, 0, 1], what
            continue
        assert counts[f][0] == len(e.matches), (what, counts[f].tolist(), len(e.matches))
        for fld in cc.FIELDS:
            assert np.array_equal(m[fld], e.matches[fld]), (what, fld)
        if mode != "similarity":
            assert dd.tobytes() == e.dd.tobytes(), (what, "depth diffs")
        if mode == "normal":
            assert nd.tobytes() == e.nd.tobytes(), (what, "normal diffs")
        if status == 2:       # side-car / range: the final matches and their diffs, no clusters
            assert counts[f].tolist() == [len(e.matches), 0, 0, 2], what
            continue
        assert counts[f].tolist() == [len(e.matches), len(e.clusters), len(e.members), 0], (what, counts[f].tolist())
        for fld in cc.CLUSTER_FIELDS:
            assert np.array_equal(c[fld], e.clusters[fld]), (what, fld)
        assert c["score"].tobytes() == e.clusters["score"].tobytes(), (what, "score bits")
        assert np.array_equal(k, e.cluster_class), (what, "cluster_class")
        assert np.array_equal(mem, e.members), (what, "members")


# ---- 1. the constructed cases through the hook ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL_CASES)
def test_constructed_case_on_the_device(name, mode):
    case = get_case(name)
    want = expected(case, mode)
    if name == "params_differ" and mode != "similarity":      # the scored modes have something to score: matches inside the scene, valid normals
        assert any((e.dd["n_valid"] > 0).any() for e in want) and (mode == "depth" or any((e.nd["n_normal"] > 0).any() for e in want))
    check_hook(case, mode, want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL_CASES)
def test_arrival_order_does_not_matter(name, mode):
    case = get_case(name)
    want = expected(case, mode)
    t = joined_object(crops_of(case), mode == "normal") if mode != "similarity" else None
    for seed in (1, 2):
        sh = ccc.shuffled(case, seed)
        assert len(sh.records) < 8 or not np.array_equal(sh.records["order_key"], case.records["order_key"])
        check_hook(sh, mode, want, templates=t)
    if t is not None:
        t.close()


def test_scored_case_reaches_what_it_is_for():
    """Case 11 on its expected values: holes and crops partly outside count, class 0's template id 2 (inside its side-car, beyond
    class_base's range) has a zero diff although index 2 of the joined object is class 1's 70 x 5 crop; a finite no_value ranks otherwise."""
    case = ccc.scored_case()
    for mode in ("depth", "normal"):
        want = expected(case, mode)
        m = np.concatenate([e.matches for e in want])
        dd = np.concatenate([e.dd for e in want])
        beyond = (m["class_index"] == 0) & (m["template_id"] == 2)
        assert beyond.sum() >= 2 and not dd["n_template"][beyond].any()
        assert (dd["n_template"][~beyond] > 0).all() and not dd["n_valid"][beyond].any()
        assert ((dd["n_valid"] > 0) & (dd["n_valid"] < dd["n_template"])).any()       # the hole, the scene's border
        wide = (m["class_index"] == 1) & (m["template_id"] == 0)
        assert wide.any() and (dd["n_template"][wide] == 350).all()            # 70 x 5, every pixel on the object
    finite = expected(case, "depth", no_value=-0.05)
    check_hook(case, "depth", finite, no_value=-0.05)
    assert any(not np.array_equal(a.clusters["score"], b.clusters["score"]) for a, b in zip(finite, expected(case, "depth")))


# ---- 2. one class: the classed kernel is the un-classed kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_one_class_equals_the_unclassed_kernel(name):
    case = cc.case_by_name(name)
    recs = case.records.copy()
    recs["class_index"] = 0
    side = (case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)
    a, ca = debug_device_finalize_cluster(recs, case.n_frames, *side, with_counts=True)
    b, cb = debug_device_finalize_cluster_classes(recs, case.n_frames, [side], with_counts=True)
    assert np.array_equal(ca, cb), (name, ca.tolist(), cb.tolist())
    for f in range(case.n_frames):
        m, c, mem, status = a[f]
        m2, _, _, c2, k2, mem2, status2 = b[f]
        assert status == status2 and m.tobytes() == m2.tobytes() and np.array_equal(mem, mem2) and not k2.any(), (name, f)
        assert len(c) == len(c2) and all(c[fld].tobytes() == c2[fld].tobytes() for fld in cc.CLUSTER_FIELDS), (name, f)


# ---- 3. lmx_depth_templates_append ------------------------------------------------------------------------------------------------------------
def test_append_moves_crops_and_normals():
    case = ccc.scored_case()
    a_crops, b_crops = case.crops[0], case.crops[1] + [np.zeros((0, 0), np.uint16)]
    a, b = DepthTemplates.from_crops(a_crops), DepthTemplates.from_crops(b_crops)
    a.enable_normals(FX, FY)
    b.enable_normals(FX, FY)
    parts_n = [a.normals(i) for i in range(len(a))] + [b.normals(i) for i in range(len(b))]
    parts_r = [a.rect(i) for i in range(len(a))] + [b.rect(i) for i in range(len(b))]
    bytes_a, bytes_b = a.device_bytes, b.device_bytes
    a.upload_scene(case.scenes)
    a.append(b)
    assert len(a) == len(a_crops) + len(b_crops) and len(b) == 0 and b.device_bytes == 0
    # the same sum of atlas, table and normals (an empty object counts nothing)
    assert a.device_bytes == bytes_a + bytes_b
    for i, want in enumerate(a_crops + b_crops):
        assert a.rect(i) == parts_r[i]
        assert np.array_equal(a.crop(i), want), i
        assert np.array_equal(a.normals(i), parts_n[i]), i
    # src is empty and valid: it takes new work and can be appended again; the scene of dst is forgotten
    with pytest.raises(_lib.LmxError):
        b.rect(0)
    assert len(b.diff(case.scenes[0], np.zeros(0, MATCH_DTYPE))) == 0
    a.append(b)
    assert len(a) == len(a_crops) + len(b_crops)
    m = np.zeros(3, MATCH_DTYPE)
    m["template_id"] = [0, 2, 4]
    m["x"], m["y"] = 5, 7
    joined = a.diff(case.scenes[0], m)
    alone = DepthTemplates.from_crops(a_crops + b_crops)
    assert joined.tobytes() == alone.diff(case.scenes[0], m).tobytes() and (joined["n_template"] > 0).all()
    with pytest.raises(_lib.LmxError) as e:
        a.append(a)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG
    for t in (a, b, alone):
        t.close()


# ---- 4. end to end on the two-class fixture ------------------------------------------------------------------------------------------------------
E2E = dict(threshold=70.0, step=32, thresh=1, rmin=0.5, rstep=0.1)


@pytest.fixture(scope="module")
def two_classes():
    path = os.path.join(ROOT, "tests", "golden", "case_rgbd_two_classes_T48.npz")
    _, bank, sources = golden_util.load(path)
    W = H = 192
    rolled = [np.ascontiguousarray(np.roll(s, (8, 16), (0, 1))) for s in sources]
    frames = [sources, rolled, sources]
    det = Detector(bank, W, H, max_batch=3)
    names = det.classIds()
    assert names == ["cpu_binary", "memoryChip2"]
    by_name = {cid: t for cid, t, _ in bank.classes}
    rows = len(bank.T) * len(bank.modalities)
    rng = np.random.default_rng(77)
    classes, crops = [], []
    for c, cid in enumerate(names):
        t = by_name[cid][::rows]
        n = len(t)
        rects = np.stack([np.zeros(n), np.zeros(n), t[:, 0], t[:, 1]], 1).astype(np.int32)
        dists = 0.55 + 0.1 * ((np.arange(n) + c) % 3) + 0.013 * c                   # different distances per class
        classes.append(ccc.Side(dists, rects, E2E["step"], E2E["rmin"], E2E["rstep"], E2E["thresh"]))
        crops.append([ramp((int(r[3]), int(r[2])), int(rng.integers(600, 1400))) for r in rects])
        det.set_cluster_sidecar_class(c, dists, rects, E2E["step"], E2E["rmin"], E2E["rstep"], E2E["thresh"])
    yield SimpleNamespace(det=det, bank=bank, frames=frames, depth=[np.ascontiguousarray(fr[1]) for fr in frames], classes=classes, crops=crops, W=W, H=H)
    det.close()


def e2e_composition(tc, per_frame, mode, no_value=-np.inf):
    """-> per frame (matches, dd, nd, clusters, cluster_class, members) from lmx_ctx_collect's lists and entry points that existed before."""
    n = len(per_frame)
    diffs = per_class_diffs(tc.crops, tc.depth[:n], per_frame, mode == "normal") if mode != "similarity" else [(None, None)] * n
    out = []
    for f in range(n):
        dd, nd = diffs[f]
        values = None if mode == "similarity" else values_of(dd, nd, no_value)
        out.append((per_frame[f], dd, nd) + composition(tc.classes, per_frame[f], values))
    return out


def assert_frame(got, want, what):
    m, dd, nd, c, k, mem = got
    wm, wdd, wnd, wc, wk, wmem = want
    assert m.tobytes() == np.ascontiguousarray(wm).astype(MATCH_DTYPE).tobytes(), (what, "matches")
    assert (dd is None) == (wdd is None) and (nd is None) == (wnd is None), what
    if wdd is not None:
        assert dd.tobytes() == wdd.tobytes(), (what, "depth diffs")
    if wnd is not None:
        assert nd.tobytes() == wnd.tobytes(), (what, "normal diffs")
    assert len(c) == len(wc), (what, len(c), len(wc))
    for fld in ("index", "rect", "member_count"):
        assert np.array_equal(c[fld], wc[fld]), (what, fld)
    assert c["score"].tobytes() == wc["score"].tobytes(), (what, "score bits")
    assert np.array_equal(k, wk), (what, "cluster_class")
    # the call's member ranges run through the whole batch; the composition's start at 0 per frame
    for a, b in zip(c, wc):
        assert np.array_equal(mem[a["member_begin"]:a["member_begin"] + a["member_count"]], wmem[b["member_begin"]:b["member_begin"] + b["member_count"]]), what


def collect_classes(tc, n, mode, t=None, no_value=-np.inf):
    if mode == "similarity":
        return tc.det.collect_clusters_classes(n)
    t.upload_scene(tc.depth[:n])
    return tc.det.collect_clusters_classes(n, t, class_base_of(tc.crops), normals=mode == "normal", no_value=no_value)


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_equals_the_composition(two_classes, mode):
    tc = two_classes
    t = joined_object(tc.crops, mode == "normal") if mode != "similarity" else None
    tc.det.upload(tc.frames)
    for n in (1, 3):
        tc.det.enqueue(n, E2E["threshold"])
        tc.det.enqueue(n, E2E["threshold"])
        want = e2e_composition(tc, tc.det.collect(n), mode)
        # the fixture reaches what this is for: both objects found, and vote bins that hold both
        m, _, _, _, k, _ = want[0]
        assert (m["class_index"] == 0).sum() > 10 and (m["class_index"] == 1).sum() > 10
        assert (k == 0).any() and (k == 1).any()
        bins = [set(zip((m["y"][m["class_index"] == c] // E2E["step"]).tolist(), (m["x"][m["class_index"] == c] // E2E["step"]).tolist())) for c in (0, 1)]
        assert len(bins[0] & bins[1]) >= 1
        got = collect_classes(tc, n, mode, t)
        for f in range(n):
            assert_frame(got[f], want[f], (mode, n, f))
    if t is not None:
        t.close()


def test_unclassed_state_is_separate(two_classes):
    """The un-classed side-car and collect_clusters next to the per-class state: neither sees the other."""
    tc = two_classes
    s = max(tc.classes, key=lambda k: len(k.dists))       # long enough for either class's template ids
    n_all = len(s.dists)
    det = Detector(tc.bank, tc.W, tc.H, max_batch=1)
    det.upload(tc.frames[:1])
    det.enqueue(1, E2E["threshold"])
    with pytest.raises(_lib.LmxError) as e:               # no class side-car: refused, the enqueue stays
        det.collect_clusters_classes(1)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "set_cluster_sidecar_class" in str(e.value)
    det.set_cluster_sidecar(s.dists[:n_all], s.rects[:n_all], s.step, s.rmin, s.rstep, s.thresh)
    with pytest.raises(_lib.LmxError):                    # the un-classed side-car is not a class side-car
        det.collect_clusters_classes(1)
    before = det.collect_clusters(1)[0]
    for c, k in enumerate(tc.classes):
        det.set_cluster_sidecar_class(c, k.dists, k.rects, k.step, k.rmin, k.rstep, k.thresh)
    det.enqueue(1, E2E["threshold"])
    after = det.collect_clusters(1)[0]
    assert before[0].tobytes() == after[0].tobytes() and all(before[1][fld].tobytes() == after[1][fld].tobytes() for fld in cc.CLUSTER_FIELDS)
    with pytest.raises(_lib.LmxError) as e:
        det.set_cluster_sidecar_class(16, s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "0 .. 15" in str(e.value) and "lmx_cluster_matches_classes" in str(e.value)
    with pytest.raises(_lib.LmxError) as e:
        det.set_cluster_sidecar_class(1, s.dists, s.rects, 0, s.rmin, s.rstep, s.thresh)
    assert "vote_row_col_step" in str(e.value)
    # removing class 1's side-car: its matches stay listed and belong to no cluster
    det.set_cluster_sidecar_class(1, [], np.zeros((0, 4), np.int32))
    det.enqueue(1, E2E["threshold"])
    m, _, _, c, k, mem = det.collect_clusters_classes(1)[0]
    assert (m["class_index"] == 1).any() and len(k) and not k.any()
    want = composition([tc.classes[0], None], m, None)
    assert len(c) == len(want[0]) and all(c[fld].tobytes() == want[0][fld].tobytes() for fld in cc.CLUSTER_FIELDS) and np.array_equal(mem[:len(want[2])], want[2])
    det.close()


def test_refusals_leave_the_enqueue_outstanding(two_classes):
    tc = two_classes
    base = class_base_of(tc.crops)
    t = joined_object(tc.crops, False)
    short = joined_object([tc.crops[0], tc.crops[1][:-1]], False)

    def refused(templates, class_base, n_frames=1, normals=False, no_value=-np.inf):
        with pytest.raises(_lib.LmxError) as e:
            tc.det.collect_clusters_classes(n_frames, templates, class_base, normals=normals, no_value=no_value)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG
        return str(e.value)

    tc.det.upload(tc.frames)
    tc.det.enqueue(1, E2E["threshold"])
    assert "no scene uploaded" in refused(t, base)
    t.upload_scene(tc.depth[:2])
    assert "holds 2 frames" in refused(t, base)
    t.upload_scene(tc.depth[:1])
    short.upload_scene(tc.depth[:1])
    assert "depth templates" in refused(short, base)                                  # class_base ends beyond the object's count
    moved = base.copy()
    moved[1] -= 1
    assert "class 0:" in refused(t, moved)                                            # a class's range differs from its side-car
    assert "class 1 has a side-car" in refused(t, base[:2].copy())
    assert "class_base[0]" in refused(t, base + 1)
    assert "enable_normals" in refused(t, base, normals=True)
    assert "not a number" in refused(t, base, no_value=float("nan"))
    assert "n_frames=2" in refused(t, base, n_frames=2)
    got = tc.det.collect_clusters_classes(1, t, base)                                 # the enqueue is still there
    assert len(got) == 1 and len(got[0][0]) > 20 and len(got[0][3]) >= 2
    with pytest.raises(_lib.LmxError):                                                # and now it is gone
        tc.det.collect_clusters_classes(1, t, base)
    t.close()
    short.close()


def test_a_frame_beyond_2048_records_is_finished_on_the_host():
    """Frame 0 leaves more than 2048 raw records (asserted on the oracle's count) and is finished on the host inside the call, frame 1
    takes the device chain; both equal the composition, with and without the depth score."""
    S = 160
    thr, n_t = 45.0, 40
    bank = synth.make_bank(n_t, seed=91, size_range=(20.0, 36.0), classes=["a", "b"])
    frames = [synth.make_scene(bank, S, S, seed=94)[0], synth.make_scene(bank, S, S, seed=93, n_instances=1)[0]]
    depth = [np.ascontiguousarray(fr[1]) for fr in frames]
    od = o.OracleDetector(bank)
    sizes = []
    for f in range(2):
        od.match(frames[f], thr)
        sizes.append(len(od.last_raw()))
    assert sizes[0] > cc.F2_MAX > sizes[1] > 0, sizes
    det = Detector(bank, S, S, max_batch=2, max_candidates=1 << 17)
    names = det.classIds()
    by_name = {cid: t for cid, t, _ in bank.classes}
    rows = len(bank.T) * len(bank.modalities)
    rng = np.random.default_rng(8)
    tc = SimpleNamespace(det=det, depth=depth, classes=[], crops=[])
    for c, cid in enumerate(names):
        t = by_name[cid][::rows]
        n = len(t)
        rects = np.stack([np.zeros(n), np.zeros(n), t[:, 0], t[:, 1]], 1).astype(np.int32)
        dists = 0.5 + 0.1 * ((np.arange(n) + c) % 4) + rng.uniform(-0.005, 0.005, n)
        tc.classes.append(ccc.Side(dists, rects, 10, 0.5, 0.1, 2))
        tc.crops.append([ramp((int(r[3]), int(r[2])), int(rng.integers(600, 1400))) for r in rects])
        det.set_cluster_sidecar_class(c, dists, rects, 10, 0.5, 0.1, 2)
    t = joined_object(tc.crops, False)
    det.upload(frames)
    for mode in ("similarity", "depth"):
        det.enqueue(2, thr)
        det.enqueue(2, thr)
        per_frame = det.collect(2, cap_total=1 << 17)
        want = e2e_composition(tc, per_frame, mode)
        if mode == "similarity":
            got = det.collect_clusters_classes(2, cap_total=1 << 17)
        else:
            t.upload_scene(depth)
            got = det.collect_clusters_classes(2, t, class_base_of(tc.crops), cap_total=1 << 17)
        for f in range(2):
            assert len(want[f][3]) > 0 and set(want[f][4].tolist()) == {0, 1}
            assert_frame(got[f], want[f], (mode, f))
    t.close()
    det.close()


# ---- 5. the C++ caller ------------------------------------------------------------------------------------------------------------------------
def test_cpp_caller_prints_what_python_computes(two_classes, tmp_path):
    """tests/cpp/cluster_classes_main.cpp (lmx::linemod::Detector::setClusterSidecar(class, ...) + collectClustersClasses on a two-class
    bank) prints the clusters the Python path computes."""
    from linemod_pose_estimation_amd import NativeBank
    tc = two_classes
    bank_yml = str(tmp_path / "bank.yml")
    NativeBank.from_bank(tc.bank).save_yaml(bank_yml)
    for k, fr in enumerate(tc.frames[0]):
        np.ascontiguousarray(fr).tofile(str(tmp_path / ("source_%d.bin" % k)))
    with open(str(tmp_path / "sidecars.txt"), "w") as fh:
        fh.write("%d\n" % len(tc.classes))
        for s in tc.classes:
            fh.write("%d %d %.17g %.17g %d\n" % (len(s.dists), s.step, s.rmin, s.rstep, s.thresh))
            fh.write(" ".join("%.17g" % v for v in s.dists) + "\n")
            fh.write(" ".join(str(int(v)) for v in s.rects.reshape(-1)) + "\n")
    exe = str(tmp_path / "cluster_classes_main")
    csrc = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cluster_classes_main.cpp"), "-o", exe, "-L", csrc, "-llmx", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([exe, bank_yml, str(tmp_path), str(tc.W), str(tc.H), "%g" % E2E["threshold"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    tc.det.upload(tc.frames[:1])
    tc.det.enqueue(1, E2E["threshold"])
    m, _, _, c, k, mem = tc.det.collect_clusters_classes(1)[0]
    lines = ["matches %d clusters %d" % (len(m), len(c))]
    for i in range(len(c)):
        b, n = int(c["member_begin"][i]), int(c["member_count"][i])
        lines.append("class %d index %d %d %d rect %d %d %d %d score %.17g members%s" % ((k[i],) + tuple(c["index"][i]) + tuple(c["rect"][i]) + (c["score"][i],
                                                                                           "".join(" %d" % v for v in mem[b:b + n]))))
    assert len(c) >= 2
    assert res.stdout.strip().split("\n") == lines
