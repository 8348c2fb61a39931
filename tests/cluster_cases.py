"""Constructed inputs for the consumer chain of match() -- std::sort + std::unique of Detector::match, then the reference's rcd_voting ->
cluster_filter -> cluster_scoring -> nonMaximaSuppressionUsingIOU -- shared by tests/test_cluster_chain_cases.py (the host path:
lmx_merge_raw + lmx_cluster_matches) and tests/test_gpu_cluster_chain.py (the device kernel k_f2_finalize_cluster through
lmx_debug_device_finalize_cluster).  Rendered scenes never deliver what these cases hold: records left of / above the origin, more
than 16 clusters of equal score, an IoU of exactly 0.4f, frames of exactly 0 / 1 / 2047 / 2048 / 2049 records, rings outside the
packed range, duplicates that are not adjacent after the sort, ties whose order depends on the insertion order.

A case is a `Case`: one record list (RAW_DTYPE, all frames interleaved, in ARRIVAL order; `order_key` carries the insertion order),
the side-car and the parameters.  `reference(case)` is independent of the library: numpy plus the real libstdc++ (the oracle's
lmo_std_sort_perm is std::sort itself) plus the oracle's function-by-function restatement of the reference's cluster chain.
Every case function asserts, on that reference alone, that the case reaches what it is for."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle as o

RAW_DTYPE = o.RAW_DTYPE
F2_MAX = 2048            # records per frame the device chain takes; beyond it the kernel reports status 1
FIELDS = ("x", "y", "similarity", "template_id", "class_index")
CLUSTER_FIELDS = ("index", "rect", "score", "member_begin", "member_count")


def Case(name, records, n_frames, dists, rects, step, rmin=0.5, rstep=0.1, thresh=2):
    return SimpleNamespace(name=name, records=np.ascontiguousarray(records, RAW_DTYPE), n_frames=n_frames, dists=np.ascontiguousarray(dists, np.float64),
                           rects=np.ascontiguousarray(rects, np.int32).reshape(-1, 4), step=step, rmin=rmin, rstep=rstep, thresh=thresh)


# ---- building records ----------------------------------------------------------------------------------------------------------------
def frame_records(rng, frame, x, y, sim, tid, cls=0):
    """One frame's records in INSERTION order (the order of the arguments).  order_key: increasing, with random gaps on both sides of
    2^32 so that both halves of the 64-bit key decide comparisons."""
    x = np.asarray(x, np.int64).reshape(-1)
    n = len(x)
    r = np.zeros(n, RAW_DTYPE)
    r["x"], r["y"], r["similarity"], r["template_id"], r["class_index"], r["frame"] = x, y, sim, tid, cls, frame
    gaps = np.where(rng.random(n) < 0.5, rng.integers(1, 1000, n), rng.integers(1, 1 << 34, n)).astype(np.uint64)
    r["order_key"] = np.cumsum(gaps, dtype=np.uint64) + np.uint64(rng.integers(0, 1 << 40))
    return r


def interleave(rng, parts):
    """All frames in one list, shuffled: the arrival order of a slot that several workgroups append to."""
    r = np.concatenate(parts) if parts else np.zeros(0, RAW_DTYPE)
    return r[rng.permutation(len(r))]


def shuffled(case, seed):
    """The same case with its record list in another arrival order."""
    c = SimpleNamespace(**vars(case))
    c.records = case.records[np.random.default_rng(seed).permutation(len(case.records))]
    return c


def draw_frame(rng, frame, n, n_t, sims, origin=(0, 0), grid=(8, 6), pitch=20, jitter=3, n_cls=2, dup=0.1):
    """n records on a coarse lattice (bins fill), few similarities and templates (many ties), a share of exact repeats (std::unique)."""
    x = origin[0] + pitch * rng.integers(0, grid[0], n) + rng.integers(0, jitter, n)
    y = origin[1] + pitch * rng.integers(0, grid[1], n) + rng.integers(0, jitter, n)
    sim = rng.choice(np.asarray(sims, np.float32), n)
    tid = rng.integers(0, n_t, n)
    cls = rng.integers(0, n_cls, n)
    if n > 1 and dup > 0:
        k = rng.integers(0, n, max(1, int(n * dup)))
        src = rng.integers(0, n, len(k))
        for a in (x, y, sim, tid, cls):
            a[k] = a[src]
    return frame_records(rng, frame, x, y, sim, tid, cls)


def sidecar(rng, n_t, rings=3, size=(8, 60)):
    dists = 0.5 + 0.1 * (np.arange(n_t) % rings) + rng.uniform(-0.005, 0.005, n_t)
    rects = np.stack([rng.integers(0, 5, n_t), rng.integers(0, 5, n_t), rng.integers(size[0], size[1], n_t), rng.integers(size[0], size[1], n_t)], 1)
    return dists, rects.astype(np.int32)


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def std_sort_perm(sim, tid):
    """The permutation libstdc++'s std::sort leaves for Match::operator< (similarity descending, template_id ascending)."""
    L = o.lib()
    L.lmo_std_sort_perm.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    L.lmo_std_sort_perm.restype = None
    sim = np.ascontiguousarray(sim, np.float32)
    tid = np.ascontiguousarray(tid, np.int32)
    perm = np.zeros(len(sim), np.int32)
    L.lmo_std_sort_perm(sim.ctypes.data, tid.ctypes.data, len(sim), perm.ctypes.data)
    return perm


def rings_of(case):
    """Depth ring per template as the reference computes it: (int)((float dist - double radius_min) / float radius_step)."""
    d = case.dists.astype(np.float32).astype(np.float64)
    return np.trunc((d - np.float64(case.rmin)) / np.float64(np.float32(case.rstep))).astype(np.int64)


def final_matches(recs):
    """Steps 1-3 on one frame's records (any order): insertion order, the real std::sort, std::unique."""
    key = recs["order_key"]
    assert len(np.unique(key)) == len(key), "order keys must be unique within a frame"
    r = recs[np.argsort(key, kind="stable")]
    r = r[std_sort_perm(r["similarity"], r["template_id"])]
    keep = np.ones(len(r), bool)
    if len(r) > 1:
        keep[1:] = ~((r["x"][1:] == r["x"][:-1]) & (r["y"][1:] == r["y"][:-1]) & (r["similarity"][1:] == r["similarity"][:-1]) &
                     (r["class_index"][1:] == r["class_index"][:-1]))
    m = np.zeros(int(keep.sum()), o.MATCH_DTYPE)
    for k in FIELDS:
        m[k] = r[k][keep]
    return m


def bins_of(case, m):
    """{y / step, x / step, ring} per match (C division truncates toward zero), int64 [n, 3]."""
    q = lambda v: (np.sign(v) * (np.abs(v) // case.step)).astype(np.int64)   # noqa: E731
    return np.stack([q(m["y"].astype(np.int64)), q(m["x"].astype(np.int64)), rings_of(case)[m["template_id"]]], 1)


def reference_frame(case, f):
    """-> namespace(n_records, matches, clusters, members, status, n_bins).  status is what the device kernel must report: 1 beyond F2_MAX
    records, 2 for a template id outside the side-car (then clusters is None: the reference would read past its arrays) or a ring
    outside +-2^18, else 0.  clusters / members are the reference's for every frame it can take, whatever the status."""
    recs = case.records[case.records["frame"] == f]
    m = final_matches(recs)
    out = SimpleNamespace(n_records=len(recs), matches=m, clusters=None, members=None, n_bins=None)
    bad_tid = bool(((m["template_id"] < 0) | (m["template_id"] >= len(case.dists))).any())
    bad_ring = False
    if not bad_tid:
        c, mem = o.cluster_matches(m, case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)
        out.clusters, out.members = c, mem[:int(c["member_count"].sum()) if len(c) else 0].copy()
        b = bins_of(case, m)
        bad_ring = bool(len(b) and ((b[:, 2] < -(1 << 18)) | (b[:, 2] >= (1 << 18))).any())
        if len(b):
            _, cnt = np.unique(b, axis=0, return_counts=True)
            out.n_bins = int((cnt > case.thresh).sum())      # clusters before the NMS
        else:
            out.n_bins = 0
    out.status = 1 if len(recs) > F2_MAX else (2 if bad_tid or bad_ring else 0)
    return out


_REFERENCES = {}


def reference(case):
    """Per frame reference of a named case, computed once per session and shared by the tests (treat as read-only)."""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = [reference_frame(case, f) for f in range(case.n_frames)]
    return _REFERENCES[case.name]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
SIMS = (91.25, 85.5, 80.0, 77.75)


def case_sizes():
    """Frames of exactly 0, 1, 2, 2047, 2048 and 2049 records in one interleaved list, plus records tagged with frame -1 and n_frames."""
    rng = np.random.default_rng(101)
    sizes = [2047, 0, 2049, 1, 2048, 2]
    dists, rects = sidecar(rng, 12)
    parts = [draw_frame(rng, f, n, 12, SIMS[:3]) for f, n in enumerate(sizes)]
    parts += [draw_frame(rng, -1, 40, 12, SIMS[:3]), draw_frame(rng, len(sizes), 40, 12, SIMS[:3])]
    case = Case("sizes", interleave(rng, parts), len(sizes), dists, rects, 10, thresh=2)
    ref = reference(case)
    assert [r.n_records for r in ref] == sizes
    assert [r.status for r in ref] == [0, 0, 1, 0, 0, 0]
    for f in (0, 4):   # the full frames lose duplicates and form several clusters
        assert F2_MAX >= ref[f].n_records > len(ref[f].matches) > 1000 and len(ref[f].clusters) > 3
    assert len(ref[1].matches) == 0 and len(ref[3].matches) == 1 and len(ref[5].matches) == 2
    return case


def case_arrival_order():
    """Many groups of records with equal (similarity, template_id) and different (x, y): the order std::sort leaves inside a group
    depends on the order it was given, so the result is right only if the insertion order was restored from order_key first."""
    rng = np.random.default_rng(102)
    dists, rects = sidecar(rng, 6)
    parts = [draw_frame(rng, 0, 420, 6, SIMS[:3], dup=0.0), draw_frame(rng, 1, 37, 6, SIMS[:2], dup=0.0)]
    case = Case("arrival_order", interleave(rng, parts), 2, dists, rects, 10, thresh=1)
    ref = reference(case)
    r0 = case.records[case.records["frame"] == 0]
    groups = 0
    for s in np.unique(r0["similarity"]):
        for t in np.unique(r0["template_id"]):
            g = r0[(r0["similarity"] == s) & (r0["template_id"] == t)]
            groups += len(np.unique(np.stack([g["x"], g["y"]], 1), axis=0)) >= 3
    assert groups >= 10
    assert [r.status for r in ref] == [0, 0] and len(ref[0].clusters) > 3
    # observable: taking the arrival order for the insertion order gives another list, in each of the shuffles the tests use
    for seed in (None, 1, 2, 3):
        rec = r0 if seed is None else shuffled(case, seed).records
        rec = rec[rec["frame"] == 0].copy()
        rec["order_key"] = np.arange(len(rec))
        wrong = final_matches(rec)
        assert len(wrong) != len(ref[0].matches) or any(not np.array_equal(wrong[k], ref[0].matches[k]) for k in FIELDS)
    return case


def case_nonadjacent_duplicates():
    """A = (x1, y1, s, tid 1), B = (x2, y2, s, tid 2), A' = (x1, y1, s, tid 3): B sorts between the equal A and A', std::unique keeps all
    three (frame 0); without B one of A, A' goes (frame 1).  Records differing only in class_index stay, only in template_id do not."""
    rng = np.random.default_rng(103)
    dists, rects = sidecar(rng, 8)
    s = 88.5
    #            x   y   sim  tid cls
    f0 = np.array([(30, 40, s, 1, 0), (70, 40, s, 2, 0), (30, 40, s, 3, 0),          # A, B, A'
                   (10, 10, 70.0, 5, 0), (10, 10, 70.0, 5, 1),                         # differ in class only: both stay
                   (50, 90, 60.0, 6, 0), (50, 90, 60.0, 7, 0), (50, 90, 60.0, 7, 0)],  # differ in template only / not at all: one stays
                  np.float64)
    f1 = f0[[0, 2, 3, 4, 5, 6, 7]]
    parts = [frame_records(rng, f, a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4]) for f, a in enumerate((f0, f1))]
    parts = [p[rng.permutation(len(p))] for p in parts]          # any insertion order
    for f, p in enumerate(parts):
        p["order_key"] = np.sort(p["order_key"])
    case = Case("nonadjacent_duplicates", interleave(rng, parts), 2, dists, rects, 10, thresh=0)
    ref = reference(case)
    assert [len(r.matches) for r in ref] == [6, 4] and [r.status for r in ref] == [0, 0]
    assert ref[0].matches["template_id"][:3].tolist() == [1, 2, 3] and len(ref[1].matches[ref[1].matches["similarity"] == np.float32(s)]) == 1
    assert sorted(ref[0].matches["class_index"][ref[0].matches["template_id"] == 5].tolist()) == [0, 1]
    return case


def case_origin():
    """Records left of and above the origin: bins by truncating division (y = -5 and y = 5 share bin 0), negative bin indices in
    std::map order, and the reference's `int /= size_t` on negative sums (a cluster of three comes out near 2^32 / 3)."""
    rng = np.random.default_rng(104)
    n_t = 6
    dists = np.full(n_t, 0.72)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), [30, 41, 35, 52, 33, 47], [28, 39, 44, 31, 50, 37]], 1)
    groups = [[(-5, -5), (3, 5)],                                  # one bin (0, 0) across the origin, sum x = -2, sum y = 0
              [(-12, -15), (-17, -11), (-13, -19)],                # bin (-1, -1), n = 3
              [(40, -5), (42, 5), (47, -9)],                       # straddles y only
              [(-8, 120), (7, 121)],                               # straddles x only, sum x = -1
              [(-700, -650), (-695, -655)], [(-699, -3), (-691, -1), (-694, -8)],
              [(-310, -420), (-301, -427), (-305, -421)], [(-1, -1), (-9, -9)],   # (-1, -1) / (-9, -9): bin 0 again -> joins the first group
              [(-450, -120), (-455, -121)], [(-230, -530), (-231, -539)], [(-100, -700), (-109, -691), (-101, -699)],
              [(-640, -640)], [(-20, -20)]]                        # singles: filtered
    x, y, sim, tid = [], [], [], []
    for g, pts in enumerate(groups):
        for (px, py) in pts:
            x.append(px); y.append(py); tid.append(int(rng.integers(0, n_t)))
            sim.append(90.0 if g % 2 == 0 else SIMS[int(rng.integers(0, 4))])     # every other group scores exactly 90: ties between clusters
    order = rng.permutation(len(x))
    rec = frame_records(rng, 0, np.asarray(x)[order], np.asarray(y)[order], np.asarray(sim)[order], np.asarray(tid)[order])
    case = Case("origin", interleave(rng, [rec]), 1, dists, rects, 10, thresh=1)
    ref = reference(case)[0]
    c, m = ref.clusters, ref.matches
    assert ref.status == 0 and 3 < ref.n_bins <= 16          # at most 16 clusters: std::sort is an insertion sort, ties stay in map order
    assert (c["rect"][:, :2] > 1 << 20).any()                # the size_t division of a negative sum
    neg = {2: 0, 3: 0}
    for cl in c:
        mem = ref.members[cl["member_begin"]:cl["member_begin"] + cl["member_count"]]
        if (m["x"][mem].sum() < 0 or m["y"][mem].sum() < 0) and int(cl["member_count"]) in neg:
            neg[int(cl["member_count"])] += 1
    assert neg[2] >= 1 and neg[3] >= 1, neg
    assert (c["index"][:, 0] < 0).any() and (c["index"][:, 1] < 0).any()
    tied_negative = 0
    for a, b in zip(c[:-1], c[1:]):
        if a["score"] == b["score"]:
            assert tuple(a["index"]) < tuple(b["index"])        # std::map order, signed
            tied_negative += a["index"][0] < 0 or a["index"][1] < 0
    assert tied_negative >= 1
    return case


def case_rings():
    """Depth rings at their truncation boundaries: dists 0.5 + 0.1 k (k = -3..9), each one float ulp either way, distances just below
    radius_min (truncation toward zero puts them into ring 0).  One side-car entry lies beyond ring 2^18 (frame 1 uses it: status 2),
    frame 2 holds a template id == n_templates (status 2; the host path refuses it)."""
    rng = np.random.default_rng(105)
    base = (0.5 + 0.1 * np.arange(-3, 10)).astype(np.float32)
    below = np.array([0.45, 0.41, 0.49, 0.4999], np.float32)
    d32 = np.concatenate([base, np.nextafter(base, np.float32(-np.inf)), np.nextafter(base, np.float32(np.inf)), below, np.array([30000.5], np.float32)])
    n_t = len(d32)
    far = n_t - 1
    dists = d32.astype(np.float64)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), rng.integers(10, 30, n_t), rng.integers(10, 30, n_t)], 1)
    nb = len(base)

    def frame(f, tids):
        # one column per k, one row per variant (exact, one ulp below, one ulp above): no rect reaches a neighbour, so every ring shows
        # in the output; the distances below radius_min sit in the column of k = 0, where they must join the cluster of ring 0
        tids = np.asarray(tids)
        col = np.where(tids < 3 * nb, tids % nb, np.where(tids < far, 3, nb + 1))
        row = np.where(tids < 3 * nb, tids // nb, 0)
        return frame_records(rng, f, 40 * col + rng.integers(0, 5, len(tids)), 30 + 100 * row + rng.integers(0, 5, len(tids)),
                             rng.choice(np.asarray(SIMS, np.float32), len(tids)), tids)

    usable = np.arange(far)
    parts = [frame(0, np.concatenate([usable, usable, usable])), frame(1, np.concatenate([usable, [far]])), frame(2, np.concatenate([usable[:20], [n_t]]))]
    case = Case("rings", interleave(rng, parts), 3, dists, rects, 10, rmin=0.5, rstep=0.1, thresh=0)
    ring = rings_of(case)
    assert ring[far] >= 1 << 18 and (ring[3 * nb:far] == 0).all() and ring.min() < 0
    assert (ring[len(base):2 * len(base)] != ring[:len(base)]).any() or (ring[2 * len(base):3 * len(base)] != ring[:len(base)]).any()   # an ulp changes a ring
    ref = reference(case)
    assert [r.status for r in ref] == [0, 2, 2] and ref[2].clusters is None and len(ref[1].clusters) > 3
    c = ref[0].clusters
    assert (c["index"][:, 2] < 0).any() and (c["index"][:, 2] > 5).any()
    merged = False       # a ring-0 cluster that holds a template from below radius_min next to one from ring 0 proper
    for cl in c[c["index"][:, 2] == 0]:
        t = ref[0].matches["template_id"][ref[0].members[cl["member_begin"]:cl["member_begin"] + cl["member_count"]]]
        merged = merged or ((dists[t] < 0.5).any() and (dists[t] >= 0.5).any())
    assert merged
    return case


def _tie_case(name, overlap, seed):
    rng = np.random.default_rng(seed)
    n_t = 5
    dists = np.full(n_t, 0.72)
    side = 30 if overlap else 20
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), np.full(n_t, side), np.full(n_t, side)], 1)
    counts = [16, 17, 40]
    parts = []
    for f, n in enumerate(counts):
        i = np.arange(n)
        if overlap:   # rows of clusters 10 px apart with 30 x 30 rects: neighbours overlap by IoU 0.5, second neighbours by 0.2
            x, y = 10 * (i % 10), 100 * (i // 10)
        else:         # 50 px apart with 20 x 20 rects: nothing overlaps
            x, y = 50 * (i % 8), 50 * (i // 8)
        p = rng.permutation(n)
        parts.append(frame_records(rng, f, x[p], y[p], rng.choice(np.asarray(SIMS[:3], np.float32), n), rng.integers(0, n_t, n)))
    case = Case(name, interleave(rng, parts), 3, dists, rects, 10, thresh=0)
    ref = reference(case)
    for f, n in enumerate(counts):
        r = ref[f]
        assert r.status == 0 and r.n_bins == n == len(r.matches)                 # one match per cluster, n clusters before the NMS
        scores = r.matches["similarity"].astype(np.float64)
        assert len(np.unique(scores)) <= 3 < n                                     # clusters share scores
        if overlap:
            assert len(r.clusters) < n                                              # suppressions happen
        else:
            assert len(r.clusters) == n
            # the clusters in std::map order, then a STABLE sort by score: what an insertion sort leaves.  libstdc++ switches to
            # introsort above 16 elements, and its partitioning reorders ties.
            b = bins_of(case, r.matches)
            order = np.lexsort((b[:, 2], b[:, 1], b[:, 0]))
            stable = order[np.argsort(-scores[order], kind="stable")]
            same = np.array_equal(r.clusters["index"], b[stable].astype(np.int32))
            assert same == (n <= 16), (n, same)
    assert ref[1].n_bins > 16 and ref[2].n_bins > 16
    return case


def case_score_ties():
    """16, 17 and 40 one-match clusters with scores from three values and no overlap: the output order is std::sort's order of ties."""
    return _tie_case("score_ties", False, 106)


def case_score_ties_overlap():
    """The same with overlapping neighbours: which of two tied clusters survives the greedy NMS depends on std::sort's order of ties."""
    return _tie_case("score_ties_overlap", True, 107)


def case_iou_boundary():
    """Two one-match clusters with 7 x 10 rects at x = 0 and x = 3: shared 40, union 100, IoU exactly 0.4f; the reference compares
    (double)0.4f > 0.4, which holds, so the lower-scored one goes.  x = 4 (IoU 3/11) stays, x = 2 (IoU 5/9) goes."""
    assert np.float32(40) / np.float32(100) == np.float32(0.4) and float(np.float32(0.4)) > 0.4
    rng = np.random.default_rng(108)
    dists, rects = [0.72], [[0, 0, 7, 10]]
    pairs = [((0, 90.0), (3, 80.0)), ((0, 90.0), (4, 80.0)), ((0, 90.0), (2, 80.0)), ((3, 90.0), (0, 80.0))]
    parts = [frame_records(rng, f, [a[0], b[0]], [0, 0], [a[1], b[1]], [0, 0]) for f, (a, b) in enumerate(pairs)]
    case = Case("iou_boundary", interleave(rng, parts), 4, dists, rects, 1, thresh=0)
    ref = reference(case)
    assert [r.n_bins for r in ref] == [2, 2, 2, 2] and [len(r.clusters) for r in ref] == [1, 2, 1, 1]
    assert [int(r.clusters["rect"][0][0]) for r in ref] == [0, 0, 0, 3] and all(r.clusters["score"][0] == 90.0 for r in ref)
    return case


def case_filter_means(thresh):
    """Clusters of thresh - 1, thresh and thresh + 1 matches: only the last kind passes `size <= thresh -> dropped`.  Sums of x, y, w, h
    that do not divide evenly (integer division), mean similarities that are not representable sums, members in vote order."""
    rng = np.random.default_rng(110 + thresh)
    n_t = 7
    dists = np.full(n_t, 0.93)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), [21, 34, 27, 40, 23, 38, 31], [37, 22, 39, 25, 33, 29, 36]], 1)
    sims = np.array([80.1, 90.3, 70.7, 85.9], np.float32)
    sizes = [s for s in (thresh - 1, thresh, thresh + 1) if s > 0] * 3
    x, y, sim, tid = [], [], [], []
    for g, s in enumerate(sizes):
        bx, by = 112 * (g % 4), 112 * (g // 4)          # bins of 16 px, clusters 112 px apart: no rect overlaps another
        off = rng.permutation(15)[:s]
        x += [bx + int(v) for v in off]; y += [by + int(v) for v in rng.permutation(15)[:s]]
        sim += [float(v) for v in rng.choice(sims, s)]; tid += [int(v) for v in rng.integers(0, n_t, s)]
    p = rng.permutation(len(x))
    rec = frame_records(rng, 0, np.asarray(x)[p], np.asarray(y)[p], np.asarray(sim)[p], np.asarray(tid)[p])
    case = Case("filter_means_thresh%d" % thresh, interleave(rng, [rec]), 1, dists, rects, 16, thresh=thresh)
    ref = reference(case)[0]
    c, m = ref.clusters, ref.matches
    assert ref.status == 0 and len(m) == sum(sizes) and len(c) == 3 and (c["member_count"] == thresh + 1).all()
    uneven = 0
    for cl in c:
        mem = ref.members[cl["member_begin"]:cl["member_begin"] + cl["member_count"]]
        assert (np.diff(mem) > 0).all()                # vote order = order in the match list
        n = len(mem)
        uneven += any(int(v) % n for v in (m["x"][mem].sum(), m["y"][mem].sum(), case.rects[m["template_id"][mem], 2].sum(), case.rects[m["template_id"][mem], 3].sum()))
    assert uneven >= 1 or thresh == 0
    return case


def cases():
    """All named cases, built once per session."""
    return _all_cases()


@functools.lru_cache(maxsize=None)
def _all_cases():
    return (case_sizes(), case_arrival_order(), case_nonadjacent_duplicates(), case_origin(), case_rings(), case_score_ties(),
            case_score_ties_overlap(), case_iou_boundary(), case_filter_means(0), case_filter_means(2), case_filter_means(3))


CASE_NAMES = ("sizes", "arrival_order", "nonadjacent_duplicates", "origin", "rings", "score_ties", "score_ties_overlap", "iou_boundary",
              "filter_means_thresh0", "filter_means_thresh2", "filter_means_thresh3")


def case_by_name(name):
    return {c.name: c for c in cases()}[name]


# ---- seeded random draws -----------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = range(240)


def random_case(seed):
    """0 .. 2048 records per frame, 1 .. 4 frames, few similarities, a coarse lattice (sometimes across the origin), steps 1 2 7 10 16,
    rects of mixed sizes, thresholds 0 .. 3.  The lattice bounds the number of clusters (<= 144), which the kernel walks on one lane."""
    rng = np.random.default_rng(1000 + seed)
    n_frames = int(rng.integers(1, 5))
    n_t = int(rng.integers(1, 20))
    n_rings = int(rng.integers(1, 4))
    dists, rects = sidecar(rng, n_t, rings=n_rings, size=(3, int(rng.choice([12, 60, 200]))))
    step = int(rng.choice([1, 2, 7, 10, 16]))
    sims = rng.choice(np.asarray(SIMS + (99.5, 60.25), np.float32), int(rng.integers(1, 5)), replace=False)
    origin = (0, 0) if rng.random() < 0.5 else (int(rng.integers(-90, 1)), int(rng.integers(-70, 1)))
    grid = (int(rng.integers(1, 9)), int(rng.integers(1, 7)))
    pitch = int(rng.choice([step, 2 * step + 1, 20, 33]))
    jitter = int(rng.choice([1, 2, 3]))
    if grid[0] * grid[1] * n_rings * jitter * jitter > 150:
        jitter = 1                                            # at most 8 x 6 lattice points x 3 rings = 144 bins
    parts = []
    for f in range(n_frames):
        kind = rng.random()
        n = int(rng.integers(0, F2_MAX + 1)) if kind < 0.25 else (int(rng.integers(0, 150)) if kind < 0.9 else int(rng.choice([0, 1, 2, 255, 256, 257, 1024, 2048])))
        parts.append(draw_frame(rng, f, n, n_t, sims, origin, grid, pitch, jitter, n_cls=int(rng.integers(1, 4)), dup=float(rng.choice([0.0, 0.1, 0.4]))))
    if rng.random() < 0.3:
        parts.append(draw_frame(rng, int(rng.choice([-1, n_frames, 1000])), 9, n_t, sims, origin, grid, pitch, jitter))
    return Case("random%d" % seed, interleave(rng, parts), n_frames, dists, rects, step, thresh=int(rng.integers(0, 4)))
