#!/usr/bin/env python3
"""Per-class match thresholds on the two-object bank: what the per-class form costs and what it buys.  Setup of scripts/two_object_chain.py:
the committed memoryChip2 and cpu_binary banks as ONE bank of two classes with a side-car per class, 640x480, 64 resident frames per batch;
every step is an enqueue followed by collect_clusters_classes and ends synchronised.
  (a) price    a uniform enqueue at 85 against a thresholds enqueue with both entries 85 (the same work through the per-class kernels)
  (b) benefit  thresholds (85 for the first class, 80 for the second) against a uniform enqueue at 80 followed by a filter on the host that
               drops the first class's matches below 85 -- what a caller without the feature has to do
The legs of a pair ALTERNATE step by step in one process; reported are the median, the quartiles and the extremes of each leg and the median
of the per-pair differences.  Before timing the results are compared: (a) to the bit; (b) by (x, y, similarity): the second class's lists
are the same, the first class's per-class list is a SUBSET of the filtered one -- the threshold also applies at the coarser pyramid levels,
so a match that ends at 85 or more after passing the coarse level between 80 and 85 exists at a uniform 80 and not at 85 (the reference's
own detector at 85 does not report it either), and a host filter on the final similarity cannot tell it apart; how many such records the
filter keeps is reported.  Raw records per frame come from one-frame enqueues of the distinct scenes (lmx_ctx_stats); a frame with more than 2048 raw records
is one the device chain hands back to the host.  Needs a GPU.
usage: class_thresholds_bench.py [--repeats 20] [--out profiles/class_thresholds.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B = 640, 480, 64
F2_MAX = 2048


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def as_set(m, fields=("x", "y", "similarity")):
    return sorted(set(zip(*(m[k].tolist() for k in fields))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--cap-total", type=int, default=1 << 18)
    ap.add_argument("--max-candidates", type=int, default=1 << 19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_thresholds.txt"))
    args = ap.parse_args()
    from linemod_pose_estimation_amd import Detector, meshsynth as ms
    names = ("memoryChip2", "cpu_binary")
    params = (8, ms.ENSENSO["radius_min"], ms.ENSENSO["radius_step"], 2)
    both, side = ms.load_banks(names)
    meshes = {n: ms.load_mesh(n) for n in names}
    grid = ms.view_grid()
    distinct = [ms.make_scene(meshes[names[0]], grid, seed=7100 + f, n_instances=2, other_tri=meshes[names[1]], n_other=2)[0] for f in range(8)]
    frames = [distinct[f % len(distinct)] for f in range(B)]
    one = Detector(both, W, H, max_batch=B, max_candidates=args.max_candidates)
    probe = Detector(both, W, H, max_batch=1, max_candidates=args.max_candidates)
    ids = one.classIds()
    for n in names:
        one.set_cluster_sidecar_class(ids.index(n), side[n][1], side[n][0], *params)
    one.upload(frames)
    hi, lo = ids[0], ids[1]
    c_hi = 0
    lines = ["# scripts/class_thresholds_bench.py: %s as one bank of two classes, %d + %d templates, %dx%d, %d resident frames per batch, %d alternating repeats per pair"
             % (" + ".join(names), len(side[names[0]][0]), len(side[names[1]][0]), W, H, B, args.repeats)]

    def step(threshold):
        one.enqueue(B, threshold)
        return one.collect_clusters_classes(B, cap_total=args.cap_total)

    def raw_per_frame(threshold):
        """Raw records of each distinct scene matched alone, and over the batch: (mean per frame, frames above F2_MAX)."""
        raw = []
        for fr in distinct:
            probe.upload([fr])
            probe.enqueue(1, threshold)
            probe.collect(1, cap_total=args.cap_total)
            raw.append(probe.stats()["raw_matches"])
        per = [raw[f % len(distinct)] for f in range(B)]
        return float(np.mean(per)), int(sum(r > F2_MAX for r in per))

    def filtered(out):
        """The host filter behind a uniform enqueue at the lower threshold: class `hi` keeps what reaches its own threshold."""
        kept = []
        for m, _, _, c, k, mem in out:
            kept.append(m[(m["class_index"] != c_hi) | (m["similarity"] >= 85.0)])
        return kept

    def timed(leg_a, leg_b):
        for _ in range(3):
            leg_a()
            leg_b()
        ta, tb = [], []
        for _ in range(args.repeats):
            s0 = time.perf_counter()
            leg_a()
            s1 = time.perf_counter()
            leg_b()
            s2 = time.perf_counter()
            ta.append(s1 - s0)
            tb.append(s2 - s1)
        return ta, tb

    # ---- (a) the price of the per-class form -----------------------------------------------------------------------------------------------
    both85 = {hi: 85.0, lo: 85.0}
    u, p = step(85.0), step(both85)
    for f in range(B):
        for x, y in zip(u[f], p[f]):
            assert (x is None and y is None) or np.array_equal(x, y), ("uniform 85 and thresholds (85, 85) differ", f)
    ta, tb = timed(lambda: step(85.0), lambda: step(both85))
    d = 1e3 * (np.asarray(tb) - np.asarray(ta))
    mean_raw, back = raw_per_frame(85.0)
    lines += ["== (a) uniform 85 against thresholds (85, 85): matches, clusters and members equal to the bit in all %d frames ==" % B,
              "    %.0f raw records per frame, %d of %d frames above %d (handed back to the host)" % (mean_raw, back, B, F2_MAX),
              "    uniform      %s" % spread(ta),
              "    per class    %s" % spread(tb),
              "    per class - uniform, pair by pair: median %+.3f ms (quartiles %+.3f .. %+.3f); the uniform leg's own interquartile range is %.3f ms"
              % (np.median(d), np.percentile(d, 25), np.percentile(d, 75), 1e3 * (np.percentile(ta, 75) - np.percentile(ta, 25)))]
    print("\n".join(lines[-5:]), flush=True)

    # ---- (b) what the feature buys ------------------------------------------------------------------------------------------------------------
    mixed = {hi: 85.0, lo: 80.0}
    u, p = filtered(step(80.0)), step(mixed)
    equal = extra = n_hi = 0
    for f in range(B):
        m = p[f][0]
        mine, theirs = set(as_set(m[m["class_index"] == c_hi])), set(as_set(u[f][u[f]["class_index"] == c_hi]))
        assert mine <= theirs, ("a match of the per-class list is missing from the filtered uniform list", f)
        assert as_set(m[m["class_index"] != c_hi]) == as_set(u[f][u[f]["class_index"] != c_hi]), ("the lower-threshold class differs", f)
        extra += len(theirs - mine)
        n_hi += len(mine)
        equal += len(m) == len(u[f]) and all(np.array_equal(m[k], u[f][k]) for k in ("x", "y", "similarity", "template_id", "class_index"))
    ta, tb = timed(lambda: filtered(step(80.0)), lambda: step(mixed))
    d = 1e3 * (np.asarray(ta) - np.asarray(tb))
    raw_u, back_u = raw_per_frame(80.0)
    raw_p, back_p = raw_per_frame(mixed)
    lines += ["== (b) thresholds (%s 85, %s 80) against uniform 80 + host filter ==" % (hi, lo),
              "    %s: the same (x, y, similarity) in all %d frames; %s: %d distinct (x, y, similarity) at its own threshold, the filter keeps %d more (they passed the coarse"
              % (lo, B, hi, n_hi, extra),
              "    level below 85, which a detector at 85 rejects there); the two lists are equal to the bit in %d of %d frames" % (equal, B),
              "    uniform 80 + filter   %.0f raw records per frame, %d of %d frames above %d (handed back to the host);  %s" % (raw_u, back_u, B, F2_MAX, spread(ta)),
              "    thresholds            %.0f raw records per frame, %d of %d frames above %d;  %s" % (raw_p, back_p, B, F2_MAX, spread(tb)),
              "    (uniform + filter) - thresholds, pair by pair: median %+.3f ms (quartiles %+.3f .. %+.3f)" % (np.median(d), np.percentile(d, 25), np.percentile(d, 75))]
    print("\n".join(lines[-6:]), flush=True)
    one.close()
    probe.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
