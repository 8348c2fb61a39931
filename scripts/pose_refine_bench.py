#!/usr/bin/env python3
"""Pose refinement of matches against the scene depth (DepthTemplates.refine_poses = lmx_pose_refine_matches, k_pose_refine) on crops of
memoryChip2 at 640x480:
  scene      16 views of the reference's grid, each rendered once more turned by 2.5 degrees about an in-image axis and moved by
             (3, -2, 4) mm: 16 frames; the templates are the 16 unperturbed views (DepthTemplates.from_mesh)
  jobs       1, 16 and 256 matches: template k at the perturbed render's silhouette corner in frame k, jittered by up to 1 px
  device     k_pose_refine's time from the object's event pairs (set_profiling), and the host clock around the call with the scene resident
             (depth_frames=None: job upload, launch, read-back, one synchronisation)
  host       the same header (csrc/lmx_pose_refine.hpp) built with g++ -O3 -ffp-contract=off, one core, the same jobs; every record must
             be equal to the device's, byte for byte
  truth      the ground-truth case of tests/pose_refine_cases.py (320x240, two renders of memoryChip2): what the numpy restatement gets
These are recorded values, not thresholds.  Needs a GPU.
usage: pose_refine_bench.py [--repeats 20] [--out profiles/pose_refine.txt]"""
import argparse
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine.txt"))
    args = ap.parse_args()
    import pose_refine_cases as prc
    from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, DepthTemplates, meshsynth as ms

    F = ms.ENSENSO["fx"]
    cam = (F, F, W / 2.0, H / 2.0)
    chip, grid = ms.load_mesh("memoryChip2"), ms.view_grid()
    views = [grid[i] for i in range(5, 2652, 166)][:16]
    turn = prc._axis_rotation((1.0, 0.6, 0.0), math.radians(2.5))
    frames, corners = [], []
    for R, d in views:
        R_b = turn @ R
        o = R_b.T @ np.array([0.003, -0.002, 0.0])
        _, depth, _, rect = ms.render_view(chip + o, R_b, d + 0.004, F, F, W, H)
        frames.append(depth)
        corners.append(rect[:2])
    t = DepthTemplates.from_mesh(chip, views, W, H, F, F)
    crops = [t.crop(k) for k in range(16)]
    rects = np.asarray([t.rect(k) for k in range(16)], np.int32)
    P = prc.make_params(cam, cam)
    kw = prc.refine_kwargs(P)
    lines = ["pose refinement, memoryChip2 crops at %d x %d (scripts/pose_refine_bench.py): recorded values, not thresholds" % (W, H),
             "crops: %d, %d .. %d object pixels (median %d); defaults: max_dist_mm %.1f, max_iterations %d, min_pairs %d, search_radius %d"
             % (len(crops), min(int((c != 0).sum()) for c in crops), max(int((c != 0).sum()) for c in crops), int(np.median([(c != 0).sum() for c in crops])),
                P["max_dist_mm"], P["max_iterations"], P["min_pairs"], P["search_radius"]), ""]

    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libprhost.so")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", prc.CSRC, "-o", so, prc.HOST_SRC])
        host = C.CDLL(so)
    vp = C.c_void_p
    host.pr_host_refine_batch.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    pads = []
    for c in crops:
        p = np.zeros((c.shape[0], (c.shape[1] + 7) // 8 * 8), np.uint16)
        p[:, :c.shape[1]] = c
        pads.append(p)
    ptrs = (C.c_void_p * 16)(*[p.ctypes.data for p in pads])
    ws, hs = np.asarray([c.shape[1] for c in crops], np.int32), np.asarray([c.shape[0] for c in crops], np.int32)
    ps = np.asarray([p.shape[1] for p in pads], np.int32)
    rxy = np.ascontiguousarray(rects[:, :2])
    vec = prc.params_vector(P)

    t.upload_scene(frames)
    rng = np.random.RandomState(4)
    for n in (1, 16, 256):
        per = max(1, n // 16)
        m = np.zeros(n, MATCH_DTYPE)
        for i in range(n):
            k = (i // per) % 16
            jit = (0, 0) if i % per == 0 else rng.randint(-1, 2, 2)
            m["x"][i], m["y"][i], m["template_id"][i], m["similarity"][i] = corners[k][0] + jit[0], corners[k][1] + jit[1], k, 90.0
        counts = np.bincount(m["template_id"], minlength=16) if n > 1 else np.asarray([1] + [0] * 15)
        offsets = np.concatenate([[0], np.cumsum(counts)])
        order = np.argsort(m["template_id"], kind="stable")
        m = m[order]
        got = t.refine_poses(m, None, offsets, rects=rects, **kw)
        wall = timed(lambda: t.refine_poses(m, None, offsets, rects=rects, **kw), args.repeats)
        t.set_profiling(True)
        for _ in range(args.repeats):
            t.refine_poses(m, None, offsets, rects=rects, **kw)
        ms_total, launches = t.kernel_times()["k_pose_refine"]
        t.set_profiling(False)
        want = np.zeros(n, POSE_REFINE_DTYPE)

        def on_host():
            for f in range(16):
                a, b = int(offsets[f]), int(offsets[f + 1])
                if a == b:
                    continue
                jobs = np.ascontiguousarray(np.stack([m["x"][a:b], m["y"][a:b], m["template_id"][a:b]], 1), np.int32)
                rc = host.pr_host_refine_batch(ptrs, ws.ctypes.data, hs.ctypes.data, ps.ctypes.data, rxy.ctypes.data, frames[f].ctypes.data, W, H, jobs.ctypes.data,
                                               b - a, vec.ctypes.data, want[a:b].ctypes.data)
                assert rc == 0
        cpu = timed(on_host, 3, warmup=1)
        assert got.tobytes() == want.tobytes(), "device and host records differ"
        passes = int((got["iterations"] + 1).sum())
        lines.append("%3d jobs: k_pose_refine %.3f ms per launch (%d launches); call with the scene resident %.3f ms (min %.3f, max %.3f); host header, one core %.1f ms"
                     % (n, ms_total / max(launches, 1), launches, wall[0] * 1e3, wall[1] * 1e3, wall[2] * 1e3, cpu[0] * 1e3))
        lines.append("          %d passes in all, statuses %s, median rms %.3f -> %.3f mm; device records equal the host's, byte for byte"
                     % (passes, np.bincount(got["status"], minlength=5).tolist(), float(np.median(got["rms_first_mm"])), float(np.median(got["rms_last_mm"]))))
    t.close()

    lines += ["", "ground-truth case of tests/pose_refine_cases.py (memoryChip2 view 7 at 320 x 240, turned by %.1f degrees, moved by %s mm), numpy restatement:"
              % (prc.GT_ANGLE_DEG, prc.GT_SHIFT_MM)]
    g = prc.ground_truth_case()
    bx, by = g["rect_b"][:2]
    for (x, y) in ((bx, by), (bx + 1, by), (bx, by + 1)):
        for it in (0, 20):
            rec, _ = prc.np_refine(prc.make_params(prc.GT_CAM, prc.GT_CAM, max_iterations=it), g["crop"], g["rect"][:2], g["scene"], x, y)
            R_obj, t_obj = prc.compose(g["R_a"], g["distance"], rec)
            e = prc.pose_errors(R_obj, t_obj, g["R_b"], g["T_b_m"])
            lines.append("  match (%d, %d), max_iterations %2d: status %d, %2d iterations, pairs %d -> %d, rms %.4f -> %.4f mm, rotation error %.4f deg, translation error %.4f mm"
                         % (x, y, it, rec["status"], rec["iterations"], rec["n_pairs_first"], rec["n_pairs_last"], rec["rms_first_mm"], rec["rms_last_mm"], e[0], e[1]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
