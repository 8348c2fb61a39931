#!/usr/bin/env python
"""What the scene's depth outlier filter costs (DepthTemplates.set_scene_filter; csrc/lmx_scene_filter.hip): the device time of
k_scene_filter_score and k_scene_filter_apply, event pairs around each launch (DepthTemplates.set_profiling), at 1 and 64 frames of
640 x 480 and three settings -- the defaults, r = 7 with k = 15 and with k = 112 -- with a new upload_scene in front of every launch; and
the same frame through the CPU build of csrc/lmx_scene_filter.hpp (tests/cpp/scene_filter_host.cpp, g++ -O3) on one core.  The frames
are tests/scene_filter_cases.noisy: a slanted surface with 0..3 mm of noise, 2 % holes and 300 pixels well in front of it.  The lines
are printed and, with --out, written: the "cost of the filter" block of profiles/scene_filter.txt.  Recorded values, not thresholds."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480
CAM = (570.0, 570.0, 320.0, 240.0)
SETTINGS = ((3, 15), (7, 15), (7, 112))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import scene_filter_cases as sfc
    from linemod_pose_estimation_amd import DepthTemplates

    distinct = [sfc.noisy(W, H, 100 + f, holes=0.02, spikes=300) for f in range(8)]
    lines = ["scene filter on frames of %d x %d (a slanted surface, 2 %% holes, 300 spikes), camera %s (scripts/scene_filter_bench.py): recorded values, not thresholds"
             % (W, H, CAM)]
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    for n in args.frames:
        frames = [distinct[f % len(distinct)] for f in range(n)]
        for r, k in SETTINGS:
            t.set_scene_filter(r, k, 1.0, camera=CAM)
            t.upload_scene(frames)
            t.debug_scene_filtered(0)           # warm-up, allocation
            t.set_profiling(True)
            for _ in range(args.repeats):
                t.upload_scene(frames)
                _, info = t.debug_scene_filtered(0)
            times = t.kernel_times()
            t.set_profiling(False)
            s, a = times["k_scene_filter_score"], times["k_scene_filter_apply"]
            assert s[1] == args.repeats and a[1] == args.repeats
            lines.append("  %2d frame(s), r %d, k %3d: k_scene_filter_score %.4f ms, k_scene_filter_apply %.4f ms a launch (mean of %d); frame 0: %d scored, %d sparse, %d removed"
                         % (n, r, k, s[0] / s[1], a[0] / a[1], args.repeats, info["n_scored"], info["n_sparse"], info["n_removed"]))
    t.close()
    with tempfile.TemporaryDirectory() as d:
        lib = sfc.build_host(d, opt="-O3")
        for r, k in SETTINGS:
            best = float("inf")
            for _ in range(3):
                t0 = time.perf_counter()
                rc, _, _ = sfc.host_filter(lib, distinct[0], CAM, r, k, 1.0)
                best = min(best, time.perf_counter() - t0)
            assert rc == 0
            lines.append("  the header on one CPU core (g++ -O3), 1 frame, r %d, k %3d: %.1f ms (best of 3)" % (r, k, best * 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
