#!/usr/bin/env python3
"""What the normal term costs, on the 2652-view memoryChip2 bank at 640x480 (the bank, renders and scenes of scripts/cluster_depth_bench.py),
1 frame and 64 frames per step:
  (a)  enqueue; DepthTemplates.upload_scene; Detector.collect_clusters_depth           the depth-scored step as it was
  (b)  enqueue; DepthTemplates.upload_scene; Detector.collect_clusters_depth_normal    the same with both terms
  (c)  the device time of k_normal_map_frames and of the walk kernels alone (DepthTemplates.set_profiling), in a pass of its own
Both legs start from frames already uploaded to the context and are timed with the host clock around one whole step, which ends in a
device synchronise.  The legs ALTERNATE step by step in one process; reported are the median, the quartiles and the extremes of each
leg and the median of the per-pair differences.  upload_scene is part of each step, so the scene's normals are computed in every (b).
  --legs a   only leg (a), using nothing this commit added: the same script then measures an older checkout of the project (run it from
             there); alternate such runs with runs of this commit on one machine to compare the two (a)s.
Needs a GPU.
usage: normal_verify_timing.py [--legs ab|a] [--threshold 80] [--repeats 40] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
HBM_PEAK_GBS = 8000.0      # MI355X: 8 TB/s


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", choices=("ab", "a"), default="ab")
    ap.add_argument("--threshold", type=float, default=80.0)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--cap-total", type=int, default=1 << 16)
    ap.add_argument("--max-candidates", type=int, default=1 << 19)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    from linemod_pose_estimation_amd import DepthTemplates, Detector, meshsynth as ms
    F = ms.ENSENSO["fx"]
    side = (8, ms.ENSENSO["radius_min"], ms.ENSENSO["radius_step"], 2)
    bank, rects, dists, view_of = ms.load_bank("memoryChip2")
    chip, cpu_mesh, grid = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary"), ms.view_grid()
    t = DepthTemplates.from_mesh(chip, [grid[int(v)] for v in view_of], W, H, F, F)
    both = args.legs == "ab"
    if both:
        t.enable_normals(F, F)
    distinct = [ms.make_scene(chip, grid, seed=7000 + f, n_instances=3, other_tri=cpu_mesh, n_other=2)[0] for f in range(16)]
    lines = ["# scripts/normal_verify_timing.py --legs %s (%s): memoryChip2, %d templates, %dx%d, threshold %g, %d repeats; templates' device bytes %d"
             % (args.legs, args.label, len(t), W, H, args.threshold, args.repeats, t.device_bytes)]
    for B in (1, 64):
        frames = [distinct[f % len(distinct)] for f in range(B)]
        depth = [np.ascontiguousarray(fr[1]) for fr in frames]
        det = Detector(bank, W, H, max_batch=B, max_candidates=args.max_candidates)
        det.set_cluster_sidecar(dists, rects, *side)
        det.upload(frames)

        def leg_a():
            det.enqueue(B, args.threshold)
            t.upload_scene(depth)
            return det.collect_clusters_depth(B, t, cap_total=args.cap_total)

        def leg_b():
            det.enqueue(B, args.threshold)
            t.upload_scene(depth)
            return det.collect_clusters_depth_normal(B, t, cap_total=args.cap_total)

        a = leg_a()
        n_matches = [len(fr[0]) for fr in a]
        if both:
            b = leg_b()
            for f in range(B):
                assert a[f][0].tobytes() == b[f][0].tobytes() and a[f][1].tobytes() == b[f][1].tobytes(), f     # matches and depth diffs
        for _ in range(3):
            leg_a()
            if both:
                leg_b()
        ta, tb = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            leg_a()
            t1 = time.perf_counter()
            if both:
                leg_b()
            t2 = time.perf_counter()
            ta.append(t1 - t0)
            tb.append(t2 - t1)
        st = det.stats()
        lines += ["%d frame%s per step: %.0f matches per frame (min %d, max %d); raw records of the last step %d"
                  % (B, "" if B == 1 else "s", np.mean(n_matches), min(n_matches), max(n_matches), st["raw_matches"]),
                  "    (a) depth         %s" % spread(ta)]
        if both:
            diff = 1e3 * (np.asarray(tb) - np.asarray(ta))
            lines += ["    (b) depth+normal  %s" % spread(tb),
                      "    (b) - (a), pair by pair: median %.3f ms (quartiles %.3f .. %.3f) = %.4f ms per frame; (a)'s own interquartile range is %.3f ms"
                      % (np.median(diff), np.percentile(diff, 25), np.percentile(diff, 75), np.median(diff) / B, 1e3 * (np.percentile(ta, 75) - np.percentile(ta, 25)))]
            # (c) the kernels alone, in a pass of their own: events around each launch
            t.set_profiling(True)
            for _ in range(10):
                leg_a()
                leg_b()
            kt = t.kernel_times()
            t.set_profiling(False)
            for name in ("k_normal_map_frames", "k_verify_diff_records", "k_depth_diff_records"):
                ms_total, n = kt[name]
                lines.append("    (c) %-22s %.4f ms per launch over %d launches" % (name, ms_total / max(n, 1), n))
            ms_map = kt["k_normal_map_frames"][0] / max(kt["k_normal_map_frames"][1], 1)
            moved = B * W * H * (2 + 8)          # each depth element read once from HBM (its eight taps come from cache), each normal written once
            lines.append("        k_normal_map_frames moves %.2f MB per launch (2 B read + 8 B written per pixel): %.0f GB/s, %.1f %% of the %.0f GB/s HBM peak"
                         % (moved / 1e6, moved / (ms_map * 1e-3) / 1e9, 100.0 * moved / (ms_map * 1e-3) / 1e9 / HBM_PEAK_GBS, HBM_PEAK_GBS))
        print("\n".join(lines), flush=True)
        det.close()
    t.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
