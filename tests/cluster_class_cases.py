"""Constructed inputs for the PER-CLASS consumer chain of a bank of several classes (lmx_cluster_matches_classes on the host, the CLASSES
forms of k_f2_finalize_cluster on the device), shared by tests/test_cluster_classes_host.py and tests/test_gpu_cluster_classes.py.

A case is a `ClassCase`: one record list as in tests/cluster_cases.py (all frames interleaved, arrival order) and one side-car per class
index (None: the class has none).  `reference(case)` is the oracle's restatement of the reference's chain applied per class, as
include/lmx.h defines the composition: for each class with a side-car, in ascending order, the chain on that class's matches (in the
list's order), member indices mapped back to the whole list, the classes' clusters joined.  Nothing of the library is in it.
Every case function asserts, on that reference alone, that the case reaches what it is for."""
import functools
from types import SimpleNamespace

import numpy as np

import cluster_cases as cc
from oracle import oracle as o

F2_MAX = cc.F2_MAX
RING_LIMIT = 1 << 16     # the classed vote key holds rings -2^16 .. 2^16 - 1; beyond that the kernel reports status 2


def Side(dists, rects, step, rmin=0.5, rstep=0.1, thresh=2):
    return SimpleNamespace(dists=np.ascontiguousarray(dists, np.float64), rects=np.ascontiguousarray(rects, np.int32).reshape(-1, 4), step=step, rmin=rmin,
                           rstep=rstep, thresh=thresh)


def ClassCase(name, records, n_frames, classes, **extra):
    return SimpleNamespace(name=name, records=np.ascontiguousarray(records, cc.RAW_DTYPE), n_frames=n_frames, classes=list(classes), **extra)


def as_tuples(case):
    """The side-cars as the Python front ends take them."""
    return [None if s is None else (s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh) for s in case.classes]


def compose(m, classes, chain):
    """The composition: chain(c, side, M_c, positions) -> (clusters, members) per class with a side-car; -> (clusters, cluster_class,
    members) with the members as positions in m."""
    cl, ccls, mem = [], [], []
    n_mem = 0
    for c, s in enumerate(classes):
        if s is None:
            continue
        pos = np.flatnonzero(m["class_index"] == c)
        k, kmem = chain(c, s, m[pos], pos)
        k = k.copy()
        for i in range(len(k)):
            b, n = int(k["member_begin"][i]), int(k["member_count"][i])
            mem.append(pos[kmem[b:b + n]].astype(np.int32))
            k["member_begin"][i] = n_mem
            n_mem += n
        cl.append(k)
        ccls.append(np.full(len(k), c, np.int32))
    clusters = np.concatenate(cl) if cl else np.zeros(0, o.CLUSTER_DTYPE)
    return clusters, (np.concatenate(ccls) if ccls else np.zeros(0, np.int32)), (np.concatenate(mem) if mem else np.zeros(0, np.int32))


def oracle_chain(c, s, mc, pos):
    return o.cluster_matches(mc, s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh)


def rings_of(s):
    d = s.dists.astype(np.float32).astype(np.float64)
    return np.trunc((d - np.float64(s.rmin)) / np.float64(np.float32(s.rstep))).astype(np.int64)


def reference_frame(case, f):
    """-> namespace(n_records, matches, clusters, cluster_class, members, status).  status as the classed kernel must report it: 1 beyond
    F2_MAX records; 2 for a match whose template id is outside ITS CLASS's side-car (clusters is None then: the host composition refuses)
    or whose ring is outside the packed range; else 0."""
    recs = case.records[case.records["frame"] == f]
    m = cc.final_matches(recs)
    out = SimpleNamespace(n_records=len(recs), matches=m, clusters=None, cluster_class=None, members=None)
    assert (m["class_index"] >= 0).all()
    bad_tid = bad_ring = False
    for c, s in enumerate(case.classes):
        if s is None:
            continue
        t = m["template_id"][m["class_index"] == c]
        if ((t < 0) | (t >= len(s.dists))).any():
            bad_tid = True
        elif len(t):
            r = rings_of(s)[t]
            bad_ring = bad_ring or bool(((r < -RING_LIMIT) | (r >= RING_LIMIT)).any())
    if not bad_tid:
        out.clusters, out.cluster_class, out.members = compose(m, case.classes, oracle_chain)
    out.status = 1 if len(recs) > F2_MAX else (2 if bad_tid or bad_ring else 0)
    return out


_REFERENCES = {}


def reference(case):
    """Per frame reference of a named case, computed once per session and shared by the tests (treat as read-only)."""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = [reference_frame(case, f) for f in range(case.n_frames)]
    return _REFERENCES[case.name]


def unclassed(case, f, side):
    """What the chain WITHOUT classes makes of frame f with one side-car: the behaviour the per-class chain replaces."""
    m = reference(case)[f].matches
    return o.cluster_matches(m, side.dists, side.rects, side.step, side.rmin, side.rstep, side.thresh)


def shuffled(case, seed):
    c = SimpleNamespace(**vars(case))
    c.records = case.records[np.random.default_rng(seed).permutation(len(case.records))]
    return c


def _rows(rng, frame, rows):
    """rows: (x, y, similarity, template_id, class) in insertion order."""
    a = np.asarray(rows, np.float64).reshape(-1, 5)
    return cc.frame_records(rng, frame, a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4])


def _members_of(r, k):
    return r.members[r.clusters["member_begin"][k]:r.clusters["member_begin"][k] + r.clusters["member_count"][k]]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def case_same_bin():
    """1. Three matches of class 0 and three of class 1 in one vote bin and ring: without classes one cluster of six, per class two of three."""
    rng = np.random.default_rng(201)
    s = Side([0.72, 0.72], [[0, 0, 30, 20], [0, 0, 30, 20]], 10, thresh=2)
    rows = [(100 + i, 101 + (i * 3) % 7, 90.0 - i, i % 2, i % 2) for i in range(6)]
    rows += [(300, 300, 70.0, 0, 0), (305, 301, 71.0, 1, 1)]          # below the size threshold in either class
    case = ClassCase("same_bin", cc.interleave(rng, [_rows(rng, 0, rows)]), 1, [s, s])
    r = reference(case)[0]
    un, _ = unclassed(case, 0, s)
    assert len(un) == 1 and un["member_count"][0] == 6
    assert r.status == 0 and len(r.clusters) == 2 and r.cluster_class.tolist() == [0, 1] and r.clusters["member_count"].tolist() == [3, 3]
    assert np.array_equal(r.clusters["index"][0], r.clusters["index"][1])                      # the same bin and ring
    for k in (0, 1):
        assert (r.matches["class_index"][_members_of(r, k)] == k).all()
    return case


def case_same_template_id():
    """2. Template id 0 exists in both classes with another rect and another origin distance: the mean rect and the ring are the class's."""
    rng = np.random.default_rng(202)
    a = Side([0.72, 0.72], [[0, 0, 30, 20], [0, 0, 32, 22]], 10, thresh=0)
    b = Side([0.95, 0.95], [[0, 0, 50, 40], [0, 0, 54, 44]], 10, thresh=0)
    rows = [(40, 40, 90.0, 0, 0), (44, 43, 88.0, 0, 0), (240, 40, 87.0, 0, 1), (243, 44, 85.0, 0, 1)]
    case = ClassCase("same_template_id", cc.interleave(rng, [_rows(rng, 0, rows)]), 1, [a, b])
    r = reference(case)[0]
    assert r.status == 0 and r.cluster_class.tolist() == [0, 1]
    assert r.clusters["rect"][0][2:].tolist() == [30, 20] and r.clusters["rect"][1][2:].tolist() == [50, 40]
    assert r.clusters["index"][0][2] == 2 and r.clusters["index"][1][2] == 4
    un, _ = unclassed(case, 0, a)                                                                 # object B measured with A's side-car
    assert sorted(un["rect"][:, 2].tolist()) == [30, 30]
    return case


def case_params_differ():
    """3. Step 8 against 20, size threshold 0 against 2, other ring constants: every parameter is the class's own."""
    rng = np.random.default_rng(203)
    da, ra = cc.sidecar(rng, 9)
    db, rb = cc.sidecar(rng, 7, rings=1)
    a, b = Side(da, ra, 8, 0.5, 0.1, 0), Side(db, rb, 20, 0.3, 0.07, 2)
    parts = [cc.draw_frame(rng, f, n, 7, cc.SIMS, grid=(4, 3), pitch=20, jitter=3, n_cls=2) for f, n in enumerate((64, 48, 40))]
    case = ClassCase("params_differ", cc.interleave(rng, parts), 3, [a, b])
    ref = reference(case)
    assert [r.status for r in ref] == [0, 0, 0]
    counts = {0: [], 1: []}
    for r in ref:
        for k in range(len(r.clusters)):
            counts[int(r.cluster_class[k])].append(int(r.clusters["member_count"][k]))
        m1 = r.matches[r.matches["class_index"] == 1]
        bins = np.stack([m1["y"] // 20, m1["x"] // 20, rings_of(b)[m1["template_id"]]], 1)
        _, cnt = np.unique(bins, axis=0, return_counts=True)
        assert (cnt <= 2).any()                                    # class 1 has bins its threshold removes
    assert min(counts[0]) == 1 and min(counts[1]) >= 3 and len(counts[1]) >= 2
    return case


def case_class_without_sidecar():
    """4. Three classes, the middle one without a side-car: its matches are listed and belong to no cluster.  Frame 1 holds only that class."""
    rng = np.random.default_rng(204)
    d, r4 = cc.sidecar(rng, 8)
    s = Side(d, r4, 10, thresh=1)
    parts = [cc.draw_frame(rng, 0, 60, 8, cc.SIMS, grid=(4, 3), n_cls=3), cc.draw_frame(rng, 1, 25, 8, cc.SIMS, grid=(3, 2), n_cls=1),
             cc.draw_frame(rng, 2, 40, 8, cc.SIMS, grid=(4, 3), n_cls=3)]
    parts[1]["class_index"] = 1
    case = ClassCase("class_without_sidecar", cc.interleave(rng, parts), 3, [s, None, s])
    ref = reference(case)
    assert [x.status for x in ref] == [0, 0, 0]
    assert len(ref[1].matches) > 10 and len(ref[1].clusters) == 0
    for f in (0, 2):
        x = ref[f]
        assert (x.matches["class_index"] == 1).sum() > 5 and set(x.cluster_class.tolist()) == {0, 2}
        assert (x.matches["class_index"][x.members] != 1).all()
        assert (np.diff(x.cluster_class) >= 0).all()
    return case


def case_nms_within_class():
    """5. Two one-match clusters with IoU 5/9: of different classes both survive (frame 0), of one class the lower-scored one goes (frame 1)."""
    rng = np.random.default_rng(205)
    s = Side([0.72], [[0, 0, 7, 10]], 1, thresh=0)
    parts = [_rows(rng, 0, [(0, 0, 90.0, 0, 0), (2, 0, 80.0, 0, 1)]), _rows(rng, 1, [(0, 0, 90.0, 0, 0), (2, 0, 80.0, 0, 0)])]
    case = ClassCase("nms_within_class", cc.interleave(rng, parts), 2, [s, s])
    ref = reference(case)
    assert [len(x.clusters) for x in ref] == [2, 1] and ref[0].cluster_class.tolist() == [0, 1] and ref[1].clusters["score"][0] == 90.0
    un, _ = unclassed(case, 0, s)
    assert len(un) == 1                                             # without classes object B is suppressed behind object A
    return case


def case_score_ties():
    """6. 20 and 25 one-match clusters in classes 0 and 1, every one with the same score, nothing overlapping: the order of each class's
    clusters is libstdc++'s std::sort of THAT class's list, which neither a stable sort nor a sort of the joined list gives."""
    rng = np.random.default_rng(206)
    s = Side(np.full(5, 0.72), np.stack([np.zeros(5), np.zeros(5), np.full(5, 20), np.full(5, 20)], 1), 10, thresh=0)
    rows = []
    for c, n in ((0, 20), (1, 25)):
        for i in rng.permutation(n):
            rows.append((50 * (i % 8) + 400 * c, 50 * (i // 8), 85.5, int(rng.integers(0, 5)), c))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    case = ClassCase("score_ties", cc.interleave(rng, [_rows(rng, 0, rows)]), 1, [s, s])
    r = reference(case)[0]
    assert r.status == 0 and (r.cluster_class == 0).sum() == 20 and (r.cluster_class == 1).sum() == 25
    for c in (0, 1):
        k = r.clusters[r.cluster_class == c]
        assert len(k) > 16 and (k["score"] == 85.5).all()                                     # more than 16 clusters of equal score
        order = np.lexsort((k["index"][:, 2], k["index"][:, 1], k["index"][:, 0]))
        stable = order[np.argsort(-k["score"][order], kind="stable")]
        assert not np.array_equal(k["index"], k["index"][stable])                          # introsort reordered ties
    un, un_members = unclassed(case, 0, s)                                                  # one sort over all 45 clusters
    assert len(un) == 45
    first = r.matches["class_index"][un_members[un["member_begin"]]]
    joined = [tuple(x) for x in un["index"][first == 0]] + [tuple(x) for x in un["index"][first == 1]]
    assert joined != [tuple(x) for x in r.clusters["index"]]
    return case


def case_sizes():
    """7. Frames of 0, 1, 2047, 2048 and 2049 records and a frame whose records are all of one class."""
    rng = np.random.default_rng(207)
    sizes = [2047, 0, 2049, 1, 2048, 300]
    da, ra = cc.sidecar(rng, 12)
    db, rb = cc.sidecar(rng, 12)
    parts = [cc.draw_frame(rng, f, n, 12, cc.SIMS[:3]) for f, n in enumerate(sizes)]
    parts[5]["class_index"] = 1
    parts.append(cc.draw_frame(rng, len(sizes), 30, 12, cc.SIMS[:3]))       # a frame beyond n_frames
    case = ClassCase("sizes", cc.interleave(rng, parts), len(sizes), [Side(da, ra, 10, thresh=2), Side(db, rb, 10, thresh=2)])
    ref = reference(case)
    assert [x.n_records for x in ref] == sizes and [x.status for x in ref] == [0, 0, 1, 0, 0, 0]
    for f in (0, 4):
        assert set(ref[f].cluster_class.tolist()) == {0, 1} and len(ref[f].clusters) > 6
    assert len(ref[3].matches) == 1 and len(ref[1].matches) == 0
    assert set(ref[5].cluster_class.tolist()) == {1} and len(ref[5].clusters) > 3
    return case


def case_ring_limits():
    """8. Rings 2^16 - 1 and 2^16, -2^16 and -2^16 - 1 in class 1 (radius_min 0, radius_step 1): status 0, 2, 0, 2."""
    rng = np.random.default_rng(208)
    d, r4 = cc.sidecar(rng, 4)
    a = Side(d, r4, 10, thresh=0)
    b = Side([65535.5, 65536.5, -65536.25, -65537.5, 3.5], np.tile([0, 0, 20, 20], (5, 1)), 10, 0.0, 1.0, 0)
    assert rings_of(b).tolist() == [65535, 65536, -65536, -65537, 3]
    parts = []
    for f, t in enumerate((0, 1, 2, 3)):
        rows = [(30, 30, 90.0, t, 1), (33, 31, 85.0, t, 1), (200, 100, 80.0, 4, 1), (60, 60, 77.0, 1, 0), (64, 63, 75.0, 2, 0)]
        parts.append(_rows(rng, f, [rows[i] for i in rng.permutation(len(rows))]))
    case = ClassCase("ring_limits", cc.interleave(rng, parts), 4, [a, b])
    ref = reference(case)
    assert [x.status for x in ref] == [0, 2, 0, 2]
    assert 65535 in ref[0].clusters["index"][:, 2].tolist() and -65536 in ref[2].clusters["index"][:, 2].tolist()
    assert all(x.clusters is not None and len(x.clusters) >= 3 for x in ref)          # the host path takes every frame
    return case


def case_class_15():
    """9. Class 15, x and y at -32768 and 32767 with step 1: the ends of every field of the vote key but the ring's."""
    rng = np.random.default_rng(209)
    s = Side([0.72, 65535.5], [[0, 0, 20, 20], [0, 0, 24, 18]], 1, 0.0, 1.0, 0)
    classes = [None] * 16
    classes[0], classes[15] = Side([0.72], [[0, 0, 20, 20]], 1, thresh=0), s
    rows = [(-32768, -32768, 90.0, 0, 15), (32767, 32767, 88.0, 1, 15), (32767, -32768, 86.0, 0, 15), (-32768, 32767, 84.0, 1, 15), (32767, 32767, 83.0, 0, 15),
            (5, 5, 82.0, 0, 0), (7, 7, 81.0, 0, 7)]
    case = ClassCase("class_15", cc.interleave(rng, [_rows(rng, 0, rows)]), 1, classes)
    r = reference(case)[0]
    assert r.status == 0 and r.cluster_class.tolist().count(15) == 4 and r.cluster_class[0] == 0     # (32767, 32767) twice: the ring-0 one is suppressed
    idx = r.clusters["index"][r.cluster_class == 15]
    assert idx[:, :2].min() == -32768 and idx[:, :2].max() == 32767 and [32767, 32767, 65535] in idx.tolist()
    assert (r.matches["class_index"] == 7).sum() == 1                                   # listed, in no cluster
    return case


def case_template_beyond_class():
    """10. A template id equal to ITS class's count and below the other class's (frame 0: status 2, the host composition refuses) and one
    beyond both (frame 2); frame 1 is complete."""
    rng = np.random.default_rng(210)
    da, ra = cc.sidecar(rng, 6)
    db, rb = cc.sidecar(rng, 3)
    a, b = Side(da, ra, 10, thresh=0), Side(db, rb, 10, thresh=0)
    base = [(20, 20, 90.0, 5, 0), (24, 22, 85.0, 2, 1), (100, 60, 80.0, 0, 1), (104, 61, 79.0, 1, 0)]
    parts = [_rows(rng, 0, base + [(150, 20, 70.0, 3, 1)]), _rows(rng, 1, base), _rows(rng, 2, base + [(150, 20, 70.0, 6, 0)])]
    case = ClassCase("template_beyond_class", cc.interleave(rng, parts), 3, [a, b])
    ref = reference(case)
    assert [x.status for x in ref] == [2, 0, 2] and ref[0].clusters is None and ref[2].clusters is None and len(ref[1].clusters) >= 2
    assert len(ref[0].matches) == 5
    return case


def cases():
    return _all_cases()


@functools.lru_cache(maxsize=None)
def _all_cases():
    return (case_same_bin(), case_same_template_id(), case_params_differ(), case_class_without_sidecar(), case_nms_within_class(), case_score_ties(),
            case_sizes(), case_ring_limits(), case_class_15(), case_template_beyond_class())


CASE_NAMES = ("same_bin", "same_template_id", "params_differ", "class_without_sidecar", "nms_within_class", "score_ties", "sizes", "ring_limits", "class_15",
              "template_beyond_class")


def case_by_name(name):
    return {c.name: c for c in cases()}[name]


# ---- 11: the scored case ------------------------------------------------------------------------------------------------------------------
SCENE_W, SCENE_H = 64, 48
CLASS_BASE = (0, 2, 5)


@functools.lru_cache(maxsize=None)
def scored_case():
    """11. Crops of 1 x 1, 9 x 3 and 70 x 5 pixels in two classes (class_base 0, 2, 5), scenes of 64 x 48 with a hole, matches whose crop
    lies partly outside the scene.  Crop 0 of class 1 (70 x 5) differs from crop 0 of class 0 (1 x 1).  Class 0's side-car holds one
    template more than it has crops: template id 2 of class 0 is inside the side-car and beyond class_base's range -- a zero diff, and
    never class 1's crop 0, which is what index class_base[0] + 2 of the joined object holds."""
    rng = np.random.default_rng(211)
    crops = [[np.full((1, 1), 700, np.uint16), rng.integers(600, 900, (3, 9)).astype(np.uint16)],
             [rng.integers(500, 1000, (5, 70)).astype(np.uint16), np.full((1, 1), 820, np.uint16), rng.integers(650, 800, (3, 9)).astype(np.uint16)]]
    crops[0][1][1, 4] = 0                                                   # a pixel off the object
    scenes = [rng.integers(550, 950, (SCENE_H, SCENE_W)).astype(np.uint16) for _ in range(2)]
    scenes[0][10:20, 12:30] = 0                                             # a hole
    a = Side([0.72, 0.81, 0.72], [[0, 0, 1, 1], [0, 0, 9, 3], [0, 0, 12, 12]], 8, thresh=0)
    b = Side([0.64, 0.72, 0.93], [[0, 0, 70, 5], [0, 0, 1, 1], [0, 0, 9, 3]], 8, thresh=0)
    parts = []
    for f in range(2):
        rows = []
        for i in range(26):
            c = int(rng.integers(0, 2))
            t = int(rng.integers(0, 3))
            x, y = int(rng.choice([-3, 2, 9, 14, 17, 40, 43, 60])), int(rng.choice([-1, 3, 11, 14, 30, 33, 46]))
            rows.append((x, y, float(rng.choice(np.asarray(cc.SIMS, np.float32))), t, c))
        parts.append(_rows(rng, f, rows))
    case = ClassCase("scored", cc.interleave(rng, parts), 2, [a, b], crops=crops, scenes=scenes, class_base=CLASS_BASE)
    ref = reference(case)
    assert [x.status for x in ref] == [0, 0]
    m = np.concatenate([x.matches for x in ref])
    assert ((m["class_index"] == 0) & (m["template_id"] == 2)).sum() >= 2                 # beyond class_base's range
    assert ((m["x"] < 0) | (m["y"] < 0)).any() and (m["x"] + 9 > SCENE_W).any()
    assert all(len(x.clusters) >= 4 and set(x.cluster_class.tolist()) == {0, 1} for x in ref)
    return case
