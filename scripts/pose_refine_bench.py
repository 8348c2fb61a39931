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
With --schedule "stride:iterations:max_dist:radius,..." (one or more; DepthTemplates.set_refine_schedule) every row is measured with and
without the schedule in this one process, the two legs alternating round by round; the device's records under the schedule are first
compared with the host header's refine_job_staged, byte for byte; passes and selected pixels per stage, the time of a pass of each stride
on the largest crop and the ground-truth errors under the schedule are recorded, into profiles/pose_refine_staged.txt.
--plain runs the rows without a schedule only, one line each with the rounds' values, and calls nothing a library without schedules
lacks; with --package-root (another checkout's root, its own built library inside) it measures that checkout: scripts/ab_pose_refine.sh
alternates two of them.
--plane SHIFT[,SHIFT...] (DepthTemplates.set_refine_plane, one point_shift per stage of the first --schedule, or of the single stage):
every row is measured point-to-point at the defaults' 20 iterations and point-to-plane at --plane-iterations, the two legs alternating
round by round; the device's records under the setting are first compared with the host header's refine_job_plane, byte for byte; the
ground-truth errors of both come from the same header.  The lines are printed, and written with --out.
These are recorded values, not thresholds.  Needs a GPU.
usage: pose_refine_bench.py [--repeats 20] [--rounds 3] [--schedule S [S ...]] [--plane K[,K..]] [--plane-iterations 5] [--plain] [--package-root DIR] [--out FILE]"""
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


def kernel_ms(t, fn, repeats):
    """k_pose_refine's device time per launch over `repeats` calls of fn, from the object's event pairs."""
    t.set_profiling(True)
    for _ in range(repeats):
        fn()
    ms_total, launches = t.kernel_times()["k_pose_refine"]
    t.set_profiling(False)
    return ms_total / max(launches, 1)


def fmt(vals):
    return "%.3f ms (rounds: %s)" % (float(np.mean(vals)), ", ".join("%.3f" % v for v in vals))


def truth_with_flying_pixels(args, prc):
    """The ground-truth case of tests/pose_refine_cases.py at its three placements, the object in front of a wall with --flying-pixels
    outline pixels seeded midway, refined by the numpy restatement on the raw scene or (--scene-filter) on the scene the numpy
    restatement of csrc/lmx_scene_filter.hpp leaves -> lines."""
    import scene_filter_cases as sfc
    g = prc.ground_truth_case()
    obj = g["scene"] != 0
    scene = np.where(obj, g["scene"], args.wall_mm).astype(np.uint16)
    near = np.zeros_like(obj)
    near[1:, :] |= obj[:-1, :]
    near[:-1, :] |= obj[1:, :]
    near[:, 1:] |= obj[:, :-1]
    near[:, :-1] |= obj[:, 1:]
    outline = np.argwhere(near & ~obj)
    pick = outline[np.linspace(0, len(outline) - 1, args.flying_pixels).astype(int)] if args.flying_pixels else outline[:0]
    mid = (int(np.median(g["scene"][obj])) + args.wall_mm) // 2
    for y, x in pick:
        scene[y, x] = mid
    lines = ["ground-truth case, the object in front of a wall at %d mm, %d outline pixels at %d mm, scene filter %s (scripts/pose_refine_bench.py --flying-pixels):"
             % (args.wall_mm, len(pick), mid, "on (r 3, k 15, 1.0)" if args.scene_filter else "off")]
    if args.scene_filter:
        scene, rec, _, _ = sfc.np_filter(scene, prc.GT_CAM)
        gone = int(sum(scene[y, x] == 0 for y, x in pick))
        lines.append("  filter: %d valid, %d sparse, %d scored, %d removed (threshold %.1f); %d of the %d seeded pixels removed, %d object pixels removed"
                     % (rec["n_valid"], rec["n_sparse"], rec["n_scored"], rec["n_removed"], rec["threshold"], gone, len(pick), int((obj & (scene == 0)).sum())))
    bx, by = g["rect_b"][:2]
    for (x, y) in ((bx, by), (bx + 1, by), (bx, by + 1)):
        rec, _ = prc.np_refine(prc.make_params(prc.GT_CAM, prc.GT_CAM), g["crop"], g["rect"][:2], scene, x, y)
        e = prc.pose_errors(*prc.compose(g["R_a"], g["distance"], rec), g["R_b"], g["T_b_m"])
        lines.append("  match (%d, %d): status %d, %2d iterations, pairs %d -> %d, rms %.4f -> %.4f mm, rotation error %.4f deg, translation error %.4f mm"
                     % (x, y, rec["status"], rec["iterations"], rec["n_pairs_first"], rec["n_pairs_last"], rec["rms_first_mm"], rec["rms_last_mm"], e[0], e[1]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs with --schedule, repetitions of a row with --plain")
    ap.add_argument("--schedule", nargs="+", default=[], help="stride:iterations:max_dist:radius,... per schedule")
    ap.add_argument("--plane", default=None, help="point_shift per stage, comma-separated: -1 point-to-point, 0..20 point-to-plane")
    ap.add_argument("--plane-iterations", type=int, default=5, help="max_iterations of the plane leg when no --schedule is given")
    ap.add_argument("--plain", action="store_true", help="only the rows without a schedule, one line each")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library are measured")
    ap.add_argument("--flying-pixels", type=int, default=0, help="only the ground-truth case, on the CPU: the object in front of a wall, this many pixels on its "
                    "outline seeded midway between the two")
    ap.add_argument("--scene-filter", action="store_true", help="with --flying-pixels: the scene goes through the depth outlier filter first (the defaults)")
    ap.add_argument("--wall-mm", type=int, default=700, help="with --flying-pixels: the depth of the wall behind the object")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.package_root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import pose_refine_cases as prc
    from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, DepthTemplates, meshsynth as ms
    if args.flying_pixels or args.scene_filter:
        text = "\n".join(truth_with_flying_pixels(args, prc)) + "\n"
        print(text)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text)
        return
    if args.out is None and not args.plane:
        args.out = os.path.join(ROOT, "profiles", "pose_refine_staged.txt" if args.schedule else "pose_refine.txt")

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
    pixels = [int((c != 0).sum()) for c in crops]
    lines = ["pose refinement, memoryChip2 crops at %d x %d (scripts/pose_refine_bench.py): recorded values, not thresholds" % (W, H),
             "crops: %d, %d .. %d object pixels (median %d); defaults: max_dist_mm %.1f, max_iterations %d, min_pairs %d, search_radius %d"
             % (len(crops), min(pixels), max(pixels), int(np.median(pixels)), P["max_dist_mm"], P["max_iterations"], P["min_pairs"], P["search_radius"]), ""]

    t.upload_scene(frames)
    rng = np.random.RandomState(4)
    rows = []
    for n in (1, 16, 256):
        per = max(1, n // 16)
        m = np.zeros(n, MATCH_DTYPE)
        for i in range(n):
            k = (i // per) % 16
            jit = (0, 0) if i % per == 0 else rng.randint(-1, 2, 2)
            m["x"][i], m["y"][i], m["template_id"][i], m["similarity"][i] = corners[k][0] + jit[0], corners[k][1] + jit[1], k, 90.0
        counts = np.bincount(m["template_id"], minlength=16) if n > 1 else np.asarray([1] + [0] * 15)
        offsets = np.concatenate([[0], np.cumsum(counts)])
        rows.append((n, m[np.argsort(m["template_id"], kind="stable")], offsets))

    if args.plain:
        for n, m, offsets in rows:
            call = lambda: t.refine_poses(m, None, offsets, rects=rects, **kw)
            call()
            vals = [kernel_ms(t, call, args.repeats) for _ in range(args.rounds)]
            print("%3d jobs: k_pose_refine without a schedule %s" % (n, fmt(vals)), flush=True)
        t.close()
        return

    if args.plane:
        import pose_refine_plane_cases as ppc
        import pose_refine_staged_cases as psc
        shifts = [int(v) for v in args.plane.split(",")]
        stages = psc.parse_schedule(args.schedule[0]) if args.schedule else None
        Pp = dict(P, max_iterations=args.plane_iterations)
        kwp = prc.refine_kwargs(Pp)
        t.enable_normals(F, F)
        with tempfile.TemporaryDirectory() as tmp:
            phost = ppc.build_host(tmp)
        normals = {}
        lines.append("point-to-point at %d iterations against point_shift [%s] %s; legs alternate round by round: %d rounds of %d launches per leg, k_pose_refine's device time per launch"
                     % (P["max_iterations"], args.plane, "under the schedule [%s]" % args.schedule[0] if stages else "at %d iterations" % args.plane_iterations, args.rounds, args.repeats))
        for n, m, offsets in rows:
            point_call = lambda: t.refine_poses(m, None, offsets, rects=rects, **kw)
            plane_call = lambda: t.refine_poses(m, None, offsets, rects=rects, **kwp)
            t.set_refine_schedule(None)
            t.set_refine_plane(None)
            point = point_call()
            t.set_refine_schedule(stages)
            t.set_refine_plane(shifts)
            got = plane_call()
            for i in list(range(0, n, max(1, n // 16)))[:16]:       # the header on the host is one core: a job of every template
                f = int(m["template_id"][i])
                if f not in normals:
                    normals[f] = ppc.scene_normals(frames[f], fx=F, fy=F)
                want = ppc.host_refine_plane(phost, Pp, stages, shifts, crops[f], rects[f, :2], frames[f], normals[f], m["x"][i], m["y"][i], POSE_REFINE_DTYPE)[0]
                assert got[i:i + 1].tobytes() == want.tobytes(), "device and host records differ under the plane setting"
            legs = {False: [], True: []}
            for _ in range(args.rounds):
                for on in (False, True):
                    t.set_refine_schedule(stages if on else None)
                    t.set_refine_plane(shifts if on else None)
                    legs[on].append(kernel_ms(t, plane_call if on else point_call, args.repeats))
            t.set_refine_schedule(None)
            t.set_refine_plane(None)
            lines.append("%3d jobs: point-to-point %s; plane %s: %.2f x" % (n, fmt(legs[False]), fmt(legs[True]), float(np.mean(legs[False]) / np.mean(legs[True]))))
            lines.append("          statuses %s -> %s, iterations median %d -> %d, median rms_last %.3f -> %.3f mm; the device's records equal the host's refine_job_plane, byte for byte"
                         % (np.bincount(point["status"], minlength=5).tolist(), np.bincount(got["status"], minlength=5).tolist(), int(np.median(point["iterations"])),
                            int(np.median(got["iterations"])), float(np.median(point["rms_last_mm"])), float(np.median(got["rms_last_mm"]))))
        t.close()
        g = prc.ground_truth_case()
        lines += ["", "ground-truth case of tests/pose_refine_cases.py, the host header (rotation error / translation error):"]
        for (x, y) in ppc.ground_truth_placements():
            out = []
            G = prc.make_params(prc.GT_CAM, prc.GT_CAM)
            for name, PP, st, sh in (("point-to-point", G, None, []), ("plane", dict(G, max_iterations=args.plane_iterations), stages, shifts)):
                rec = ppc.host_refine_plane(phost, PP, st, sh, g["crop"], g["rect"][:2], g["scene"], ppc.ground_truth_normals(), x, y, POSE_REFINE_DTYPE)[0][0]
                e = prc.pose_errors(*prc.compose(g["R_a"], g["distance"], rec), g["R_b"], g["T_b_m"])
                out.append("%s: %d iterations, %.4f deg / %.4f mm" % (name, rec["iterations"], e[0], e[1]))
            lines.append("  match (%d, %d): %s" % (x, y, "; ".join(out)))
        text = "\n".join(lines) + "\n"
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return

    vp = C.c_void_p
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libprhost.so")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", prc.CSRC, "-o", so, prc.HOST_SRC])
        host = C.CDLL(so)
        if args.schedule:
            import pose_refine_staged_cases as psc
            so = os.path.join(tmp, "libprshost.so")
            subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", prc.CSRC, "-o", so, psc.HOST_SRC])
            shost = C.CDLL(so)
            shost.prs_host_refine_batch.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp]
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

    def on_host(m, offsets, want, stages=None):
        svec = psc.schedule_vector(stages) if stages else None
        for f in range(16):
            a, b = int(offsets[f]), int(offsets[f + 1])
            if a == b:
                continue
            jobs = np.ascontiguousarray(np.stack([m["x"][a:b], m["y"][a:b], m["template_id"][a:b]], 1), np.int32)
            if stages:
                rc = shost.prs_host_refine_batch(ptrs, ws.ctypes.data, hs.ctypes.data, ps.ctypes.data, rxy.ctypes.data, frames[f].ctypes.data, W, H, jobs.ctypes.data,
                                                 b - a, vec.ctypes.data, svec.ctypes.data, len(stages), want[a:b].ctypes.data)
            else:
                rc = host.pr_host_refine_batch(ptrs, ws.ctypes.data, hs.ctypes.data, ps.ctypes.data, rxy.ctypes.data, frames[f].ctypes.data, W, H, jobs.ctypes.data,
                                               b - a, vec.ctypes.data, want[a:b].ctypes.data)
            assert rc == 0

    if not args.schedule:
        for n, m, offsets in rows:
            call = lambda: t.refine_poses(m, None, offsets, rects=rects, **kw)
            got = call()
            wall = timed(call, args.repeats)
            per_launch = kernel_ms(t, call, args.repeats)
            want = np.zeros(n, POSE_REFINE_DTYPE)
            cpu = timed(lambda: on_host(m, offsets, want), 3, warmup=1)
            assert got.tobytes() == want.tobytes(), "device and host records differ"
            passes = int((got["iterations"] + 1).sum())
            lines.append("%3d jobs: k_pose_refine %.3f ms per launch (%d launches); call with the scene resident %.3f ms (min %.3f, max %.3f); host header, one core %.1f ms"
                         % (n, per_launch, args.repeats, wall[0] * 1e3, wall[1] * 1e3, wall[2] * 1e3, cpu[0] * 1e3))
            lines.append("          %d passes in all, statuses %s, median rms %.3f -> %.3f mm; device records equal the host's, byte for byte"
                         % (passes, np.bincount(got["status"], minlength=5).tolist(), float(np.median(got["rms_first_mm"])), float(np.median(got["rms_last_mm"]))))
    else:
        big = int(np.argmax(pixels))
        lines.append("legs alternate round by round in one process: %d rounds of %d launches per leg; k_pose_refine's device time per launch, mean over the rounds" % (args.rounds, args.repeats))
        for text in args.schedule:
            stages = psc.parse_schedule(text)
            lines += ["", "schedule [%s]" % text]
            for n, m, offsets in rows:
                call = lambda: t.refine_poses(m, None, offsets, rects=rects, **kw)
                t.set_refine_schedule(None)
                plain = call()
                t.set_refine_schedule(stages)
                got = call()
                want = np.zeros(n, POSE_REFINE_DTYPE)
                on_host(m, offsets, want, stages)
                assert got.tobytes() == want.tobytes(), "device and host records differ under the schedule"
                legs = {False: [], True: []}
                for _ in range(args.rounds):
                    for on in (False, True):
                        t.set_refine_schedule(stages if on else None)
                        legs[on].append(kernel_ms(t, call, args.repeats))
                t.set_refine_schedule(None)
                lines.append("%3d jobs: without a schedule %s; with it %s: %.2f x" % (n, fmt(legs[False]), fmt(legs[True]), float(np.mean(legs[False]) / np.mean(legs[True]))))
                lines.append("          statuses %s -> %s (finished in stage %s), iterations median %d -> %d, median rms_last %.3f -> %.3f mm; device records equal the host's refine_job_staged, byte for byte"
                             % (np.bincount(plain["status"], minlength=5).tolist(), np.bincount(got["status"], minlength=5).tolist(), np.bincount(got["reserved"], minlength=len(stages)).tolist(),
                                int(np.median(plain["iterations"])), int(np.median(got["iterations"])), float(np.median(plain["rms_last_mm"])), float(np.median(got["rms_last_mm"]))))
            # the largest crop's job: passes and selected pixels per stage from the numpy restatement's trace
            k = big
            rec, _, trace = psc.np_refine_staged(P, stages, crops[k], rects[k, :2], frames[k], corners[k][0], corners[k][1])
            per_stage = ["stage %d (stride %d): %d passes of %d pixels" % (s, st["stride"], sum(1 for a, _ in trace if a == s), next((px for a, px in trace if a == s), 0))
                         for s, st in enumerate(stages)]
            lines.append("          the %d-pixel crop's job: %s; %.2f full-pass equivalents of pixel work (21 without a schedule)"
                         % (pixels[k], "; ".join(per_stage), sum(px for _, px in trace) / pixels[k]))
        # a pass of each stride on the largest crop: one stage of that stride with eps 0, 4 against 20 iterations (5 and 21 passes), the difference over 16
        lines += ["", "time per pass on the %d-pixel crop (one job, one stage of the stride, eps 0: (time at 20 iterations - time at 4) / 16), rounds alternating over the strides:" % pixels[big]]
        m1 = np.zeros(1, MATCH_DTYPE)
        m1["x"], m1["y"], m1["template_id"], m1["similarity"] = corners[big][0], corners[big][1], big, 90.0
        off1 = np.asarray([0] * (big + 1) + [1] * (16 - big))
        call1 = lambda: t.refine_poses(m1, None, off1, rects=rects, **kw)
        per_pass = {g: [] for g in (1, 2, 4, 8)}
        for _ in range(args.rounds):
            for g in per_pass:
                ms_at = {}
                for it in (4, 20):
                    t.set_refine_schedule([psc.make_stage(eps_rot_rad=0.0, eps_trans_mm=0.0, max_iterations=it, stride=g)])
                    assert call1()["iterations"][0] == it
                    ms_at[it] = kernel_ms(t, call1, args.repeats)
                per_pass[g].append((ms_at[20] - ms_at[4]) / 16.0)
        t.set_refine_schedule(None)
        sel = {g: int((crops[big][::g, ::g] != 0).sum()) for g in per_pass}
        for g in per_pass:
            lines.append("  stride %d: %5d selected pixels (%.1f a lane), %s a pass; a stride-1 pass takes %.1f x as long"
                         % (g, sel[g], sel[g] / 256.0, fmt(per_pass[g]), float(np.mean(per_pass[1]) / np.mean(per_pass[g]))))
    t.close()

    lines += ["", "ground-truth case of tests/pose_refine_cases.py (memoryChip2 view 7 at 320 x 240, turned by %.1f degrees, moved by %s mm), numpy restatement:"
              % (prc.GT_ANGLE_DEG, prc.GT_SHIFT_MM)]
    g = prc.ground_truth_case()
    bx, by = g["rect_b"][:2]
    npx = int((g["crop"] != 0).sum())
    for (x, y) in ((bx, by), (bx + 1, by), (bx, by + 1)):
        for it in (0, 20):
            rec, _ = prc.np_refine(prc.make_params(prc.GT_CAM, prc.GT_CAM, max_iterations=it), g["crop"], g["rect"][:2], g["scene"], x, y)
            R_obj, t_obj = prc.compose(g["R_a"], g["distance"], rec)
            e = prc.pose_errors(R_obj, t_obj, g["R_b"], g["T_b_m"])
            lines.append("  match (%d, %d), max_iterations %2d: status %d, %2d iterations, pairs %d -> %d, rms %.4f -> %.4f mm, rotation error %.4f deg, translation error %.4f mm"
                         % (x, y, it, rec["status"], rec["iterations"], rec["n_pairs_first"], rec["n_pairs_last"], rec["rms_first_mm"], rec["rms_last_mm"], e[0], e[1]))
        for text in args.schedule:
            rec, _, trace = psc.np_refine_staged(prc.make_params(prc.GT_CAM, prc.GT_CAM), psc.parse_schedule(text), g["crop"], g["rect"][:2], g["scene"], x, y)
            e = prc.pose_errors(*prc.compose(g["R_a"], g["distance"], rec), g["R_b"], g["T_b_m"])
            lines.append("  match (%d, %d), [%s]: status %d in stage %d, %2d iterations, %.2f full passes of pixel work, pairs %d -> %d, rms %.4f -> %.4f mm, rotation error %.4f deg, "
                         "translation error %.4f mm" % (x, y, text, rec["status"], rec["reserved"], rec["iterations"], sum(px for _, px in trace) / npx, rec["n_pairs_first"],
                                                        rec["n_pairs_last"], rec["rms_first_mm"], rec["rms_last_mm"], e[0], e[1]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
