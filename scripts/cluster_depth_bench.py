#!/usr/bin/env python3
"""Depth-scored clusters: the three-call composition against the fused call, on the 2652-view memoryChip2 bank at 640x480 (the bank and
the renders of scripts/depth_verify_bench.py), 1 frame and 64 frames per call.
  composition  enqueue; collect; DepthTemplates.diff; cluster_matches_scored per frame        (two synchronisations, the host's sorts)
  fused        enqueue; DepthTemplates.upload_scene; Detector.collect_clusters_depth          (one synchronisation)
Both legs start from frames already uploaded to the context (the upload is the same for both) and are timed with the host clock around
one whole step, which ends in a device synchronise in either leg.  The legs ALTERNATE step by step in one process; reported are the
median, the quartiles and the extremes of each leg, and the median of the per-pair differences.  Before timing, the two legs' results
are compared bit for bit.  Both legs are Python callers: the composition makes 2 + n_frames library calls (one cluster call per frame) and
slices arrays in between, the fused leg makes two; the composition's three parts are timed separately so that the share of the per-frame
loop, which a C caller would run without an interpreter, can be read off.  Every threshold given is measured, one after the other, on the
same bank and frames.  Needs a GPU.
usage: cluster_depth_bench.py [--threshold 78 80 85] [--repeats 40] [--out profiles/r08_cluster_depth.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, nargs="+", default=[78.0, 80.0, 85.0])
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--cap-total", type=int, default=1 << 16, help="output capacity of a call; the fused leg allocates its outputs per call, so keep it no larger than needed")
    ap.add_argument("--max-candidates", type=int, default=1 << 19)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from linemod_pose_estimation_amd import DepthTemplates, Detector, cluster_matches_scored, depth_values, meshsynth as ms
    F = ms.ENSENSO["fx"]
    side = (8, ms.ENSENSO["radius_min"], ms.ENSENSO["radius_step"], 2)
    bank, rects, dists, view_of = ms.load_bank("memoryChip2")
    chip, cpu_mesh, grid = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary"), ms.view_grid()
    t = DepthTemplates.from_mesh(chip, [grid[int(v)] for v in view_of], W, H, F, F)
    assert len(t) == len(rects) == 2652
    distinct = [ms.make_scene(chip, grid, seed=7000 + f, n_instances=3, other_tri=cpu_mesh, n_other=2)[0] for f in range(16)]
    lines = ["# scripts/cluster_depth_bench.py: memoryChip2, %d templates, %dx%d, thresholds %s, %d alternating repeats per threshold and size"
             % (len(t), W, H, " ".join("%g" % th for th in args.threshold), args.repeats)]

    for threshold in args.threshold:
        lines.append("== threshold %g ==" % threshold)
        for B in (1, 64):
            frames = [distinct[f % len(distinct)] for f in range(B)]
            depth = [np.ascontiguousarray(fr[1]) for fr in frames]
            det = Detector(bank, W, H, max_batch=B, max_candidates=args.max_candidates)
            det.set_cluster_sidecar(dists, rects, *side)
            det.upload(frames)
            parts = []

            def composition():
                t0 = time.perf_counter()
                det.enqueue(B, threshold)
                per_frame = det.collect(B, args.cap_total)
                t1 = time.perf_counter()
                offsets = np.concatenate([[0], np.cumsum([len(m) for m in per_frame])])
                d = t.diff(depth, np.concatenate(per_frame), offsets)
                t2 = time.perf_counter()
                out = [(per_frame[f], d[offsets[f]:offsets[f + 1]]) + cluster_matches_scored(per_frame[f], depth_values(d[offsets[f]:offsets[f + 1]]), dists, rects, *side)
                       for f in range(B)]
                parts.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
                return out

            def fused():
                det.enqueue(B, threshold)
                t.upload_scene(depth)
                return det.collect_clusters_depth(B, t, cap_total=args.cap_total)

            try:
                a, b = composition(), fused()
            except Exception as e:   # a list of the context overflowed: report it and go on with the next size
                lines.append("%d frame%s per call: not measured: %s" % (B, "" if B == 1 else "s", str(e)[:200]))
                print(lines[-1], flush=True)
                det.close()
                continue
            n_matches, n_clusters = [], []
            for f in range(B):
                (m0, d0, c0, mem0), (m1, d1, c1, mem1) = a[f], b[f]
                assert m0.tobytes() == m1.tobytes() and d0.tobytes() == d1.tobytes() and len(c0) == len(c1), f
                for k in ("index", "rect", "score", "member_count"):
                    assert c0[k].tobytes() == c1[k].tobytes(), (f, k)
                for x, y in zip(c0, c1):
                    assert np.array_equal(mem0[x["member_begin"]:x["member_begin"] + x["member_count"]], mem1[y["member_begin"]:y["member_begin"] + y["member_count"]]), f
                n_matches.append(len(m0))
                n_clusters.append(len(c0))
            for _ in range(3):
                composition()
                fused()
            del parts[:]
            tc, tf = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                composition()
                t1 = time.perf_counter()
                fused()
                t2 = time.perf_counter()
                tc.append(t1 - t0)
                tf.append(t2 - t1)
            st = det.stats()
            cs = det.chain_stats()      # of the last fused call
            diff = 1e3 * (np.asarray(tc) - np.asarray(tf))
            iqr = 1e3 * (np.percentile(tc, 75) - np.percentile(tc, 25))
            part = 1e3 * np.median(np.asarray(parts), axis=0)
            lines += ["%d frame%s per call: %.0f matches and %.1f clusters per frame (min %d, max %d matches; raw records of the last call %d); results equal bit for bit"
                      % (B, "" if B == 1 else "s", np.mean(n_matches), np.mean(n_clusters), min(n_matches), max(n_matches), st["raw_matches"]),
                      "    composition  %s" % spread(tc),
                      "                 of it, medians: enqueue + collect %.3f ms, DepthTemplates.diff %.3f ms, the per-frame cluster_matches_scored loop %.3f ms"
                      % (part[0], part[1], part[2]),
                      "    fused        %s" % spread(tf),
                      "                 its frames by path: LDS kernel %d, large-frame kernel %d, host for the record count %d, host for side-car / range %d; "
                      "largest frame beyond 2048 records: %d; large-path workspace %.1f MB"
                      % (cs["frames_lds"], cs["frames_large"], cs["frames_host_records"], cs["frames_host_other"], cs["max_frame_records"], cs["large_workspace_bytes"] / 1e6),
                      "    composition - fused, pair by pair: median %.3f ms (quartiles %.3f .. %.3f); the composition's own interquartile range is %.3f ms"
                      % (np.median(diff), np.percentile(diff, 25), np.percentile(diff, 75), iqr)]
            print("\n".join(lines[-6:]), flush=True)
            det.close()
    t.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
