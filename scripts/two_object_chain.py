#!/usr/bin/env python3
"""Two objects against one camera frame: two single-class contexts against one two-class context, on the committed memoryChip2 and
cpu_binary banks (2652 + the second mesh's views) at 640x480, 64 resident frames per batch.
  two contexts  per object a context of its own with that object's bank and side-car: enqueue on both, then collect_clusters on both
                (two quantiser passes per frame, two consumer chains)
  one context   one bank of two classes with a side-car per class: enqueue, then collect_clusters_classes
                (one quantiser pass per frame, one per-class consumer chain)
Both legs start from frames already uploaded and are timed with the host clock around one whole step, which ends synchronised in either
leg.  The legs ALTERNATE step by step in one process; reported are the median, the quartiles and the extremes of each leg and the median
of the per-pair differences.  Before timing the results are compared: per class the one-context leg's matches are the single-class
context's by (x, y, similarity) (the order of ties is the one std::sort's over all classes, so which template of an adjacent duplicate
std::unique keeps may differ), and the clusters are compared by vote bin, rect and member count, with the number of frames whose lists
are equal to the bit reported next to it.  Needs a GPU.
What the numbers say is written where they are used: DESIGN.md section 7, INTEGRATION.md section 3f.
usage: two_object_chain.py [--threshold 80 85] [--repeats 20] [--out profiles/two_object_chain.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B = 640, 480, 64


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def as_set(m, fields=("x", "y", "similarity", "template_id")):
    return sorted(set(zip(*(m[k].tolist() for k in fields))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, nargs="+", default=[80.0, 85.0])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--cap-total", type=int, default=1 << 18)
    ap.add_argument("--max-candidates", type=int, default=1 << 19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_object_chain.txt"))
    args = ap.parse_args()
    from linemod_pose_estimation_amd import Detector, meshsynth as ms
    names = ("memoryChip2", "cpu_binary")
    params = (8, ms.ENSENSO["radius_min"], ms.ENSENSO["radius_step"], 2)
    both, side = ms.load_banks(names)
    single = {n: ms.load_bank(n)[0] for n in names}
    meshes = {n: ms.load_mesh(n) for n in names}
    grid = ms.view_grid()
    distinct = [ms.make_scene(meshes[names[0]], grid, seed=7100 + f, n_instances=2, other_tri=meshes[names[1]], n_other=2)[0] for f in range(8)]
    frames = [distinct[f % len(distinct)] for f in range(B)]
    lines = ["# scripts/two_object_chain.py: %s, %d + %d templates, %dx%d, %d resident frames per batch, %d alternating repeats per threshold"
             % (" + ".join(names), len(side[names[0]][0]), len(side[names[1]][0]), W, H, B, args.repeats)]

    dets = {}
    for n in names:
        dets[n] = Detector(single[n], W, H, max_batch=B, max_candidates=args.max_candidates)
        dets[n].set_cluster_sidecar(side[n][1], side[n][0], *params)
        dets[n].upload(frames)
    one = Detector(both, W, H, max_batch=B, max_candidates=args.max_candidates)
    class_of = {n: one.classIds().index(n) for n in names}
    for n in names:
        one.set_cluster_sidecar_class(class_of[n], side[n][1], side[n][0], *params)
    one.upload(frames)

    for threshold in args.threshold:
        lines.append("== threshold %g ==" % threshold)

        def two_contexts():
            for n in names:
                dets[n].enqueue(B, threshold)
            return {n: dets[n].collect_clusters(B, args.cap_total) for n in names}

        def one_context():
            one.enqueue(B, threshold)
            return one.collect_clusters_classes(B, cap_total=args.cap_total)

        try:
            a, b = two_contexts(), one_context()
        except Exception as e:   # a list of a context overflowed: report it and go on with the next threshold
            lines.append("not measured: %s" % str(e)[:200])
            print(lines[-1], flush=True)
            for d in list(dets.values()) + [one]:
                d.sync()             # lmx_ctx_sync abandons the enqueues the failed step left uncollected (outstanding = 0)
            continue
        n_matches, n_clusters, equal_bits, equal_bins, equal_lists = [], [], 0, 0, 0
        for f in range(B):
            m, _, _, c, k, mem = b[f]
            bits = bins = lists = True
            for n in names:
                m1, c1, _ = a[n][f]
                sel = m["class_index"] == class_of[n]
                # std::unique removes ADJACENT duplicates of (x, y, similarity, class), and the other class's records sort in between: which
                # template of a duplicate survives, and whether both do, may differ; every (x, y, similarity) of a class is in both
                assert as_set(m[sel], ("x", "y", "similarity")) == as_set(m1, ("x", "y", "similarity")), (threshold, f, n)
                lists = lists and as_set(m[sel]) == as_set(m1) and int(sel.sum()) == len(m1)
                mine = c[k == class_of[n]]
                key = lambda q: sorted(zip(map(tuple, q["index"].tolist()), map(tuple, q["rect"].tolist()), q["member_count"].tolist()))   # noqa: E731
                bins = bins and key(mine) == key(c1)
                bits = bits and all(mine[fld].tobytes() == c1[fld].tobytes() for fld in ("index", "rect", "score", "member_count"))
            equal_bits += bits
            equal_bins += bins
            equal_lists += lists
            n_matches.append(len(m))
            n_clusters.append(len(c))
        for _ in range(3):
            two_contexts()
            one_context()
        t2, t1 = [], []
        for _ in range(args.repeats):
            s0 = time.perf_counter()
            two_contexts()
            s1 = time.perf_counter()
            one_context()
            s2 = time.perf_counter()
            t2.append(s1 - s0)
            t1.append(s2 - s1)
        diff = 1e3 * (np.asarray(t2) - np.asarray(t1))
        iqr = 1e3 * (np.percentile(t2, 75) - np.percentile(t2, 25))
        lines += ["%.0f matches and %.1f clusters per frame over both objects (min %d, max %d matches); per class the same (x, y, similarity) in all %d frames,"
                  % (np.mean(n_matches), np.mean(n_clusters), min(n_matches), max(n_matches), B),
                  "    the same matches, template ids included, in %d frames;" % equal_lists,
                  "    cluster lists equal by bin, rect and member count in %d frames, to the bit (order and score included) in %d" % (equal_bins, equal_bits),
                  "    two contexts  %s" % spread(t2),
                  "    one context   %s" % spread(t1),
                  "    two contexts - one context, pair by pair: median %.3f ms (quartiles %.3f .. %.3f); the two-context leg's own interquartile range is %.3f ms"
                  % (np.median(diff), np.percentile(diff, 25), np.percentile(diff, 75), iqr)]
        print("\n".join(lines[-6:]), flush=True)
    for d in list(dets.values()) + [one]:
        d.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
