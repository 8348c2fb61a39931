#!/usr/bin/env python3
"""Pose verification of the cluster leaders of one 64-frame step (DepthTemplates.verify_poses = lmx_pose_verify_matches, k_pose_verify)
on the 2652-view memoryChip2 bank at 640x480 (the bank, renders and frames of scripts/cluster_depth_bench.py):
  step       enqueue; upload_scene; collect_clusters_depth at the given threshold; per cluster its leader; refine_poses on the resident
             scene: the jobs are (leader, refined pose), the scene stays resident
  device     the host clock around verify_poses(depth_frames=None), which uploads the jobs, launches once, reads the records back and
             synchronises; after warm-up calls, `repeats` calls, median, quartiles and extremes; in a second loop of its own
             k_pose_verify's time from the object's event pairs (set_profiling)
  host       the same header (csrc/lmx_pose_verify.hpp) built with g++ -O3 -ffp-contract=off, one core, the same jobs, frame by frame;
             every record must equal the device's, byte for byte
These are recorded values, not thresholds.  Needs a GPU.
usage: pose_verify_bench.py [--threshold 80] [--repeats 1000] [--out profiles/pose_verify.txt]"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480
B = 64


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def host_jobs(host, crops, rects, frames, offsets, m, poses, P, dtype):
    """The header on one core, frame by frame -> a function that fills and returns the records."""
    import pose_verify_cases as pvc
    pads = []
    for c in crops:
        p = np.zeros((c.shape[0], (c.shape[1] + 7) // 8 * 8), np.uint16)
        p[:, :c.shape[1]] = c
        pads.append(p)
    ptrs = (C.c_void_p * len(pads))(*[p.ctypes.data for p in pads])
    ws, hs = np.asarray([c.shape[1] for c in crops], np.int32), np.asarray([c.shape[0] for c in crops], np.int32)
    ps = np.asarray([p.shape[1] for p in pads], np.int32)
    rxy = np.ascontiguousarray(np.asarray(rects, np.int32)[:, :2])
    vec = pvc.params_vector(P)
    pose12 = np.ascontiguousarray(np.concatenate([poses["R"], poses["t_mm"]], 1), np.float64)
    ids = np.ascontiguousarray(m["template_id"], np.int32)
    want = np.zeros(len(m), dtype)
    keep = (pads, ptrs, ws, hs, ps, rxy, vec, pose12, ids)

    def run():
        for f in range(len(frames)):
            a, b = int(offsets[f]), int(offsets[f + 1])
            if a == b:
                continue
            rc = host.pv_host_verify_batch(ptrs, ws.ctypes.data, hs.ctypes.data, ps.ctypes.data, rxy.ctypes.data, frames[f].ctypes.data, W, H, ids[a:b].ctypes.data,
                                           pose12[a:b].ctypes.data, b - a, vec.ctypes.data, want[a:b].ctypes.data)
            assert rc == 0
        return want
    run.keep = keep
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, default=80.0)
    ap.add_argument("--repeats", type=int, default=1000, help="calls in the timed window: enough of them that the window is a good part of a second")
    ap.add_argument("--cap-total", type=int, default=1 << 16)
    ap.add_argument("--max-candidates", type=int, default=1 << 19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_verify.txt"))
    args = ap.parse_args()
    import pose_verify_cases as pvc
    from linemod_pose_estimation_amd import POSE_VERIFY_DTYPE, DepthTemplates, Detector, cluster_leaders, keep_verified, meshsynth as ms

    F = ms.ENSENSO["fx"]
    cam = (F, F, W / 2.0, H / 2.0)
    side = (8, ms.ENSENSO["radius_min"], ms.ENSENSO["radius_step"], 2)
    bank, rects, dists, view_of = ms.load_bank("memoryChip2")
    chip, cpu_mesh, grid = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary"), ms.view_grid()
    t = DepthTemplates.from_mesh(chip, [grid[int(v)] for v in view_of], W, H, F, F)
    distinct = [ms.make_scene(chip, grid, seed=7000 + f, n_instances=3, other_tri=cpu_mesh, n_other=2)[0] for f in range(16)]
    frames = [distinct[f % len(distinct)] for f in range(B)]
    depth = [np.ascontiguousarray(fr[1]) for fr in frames]
    det = Detector(bank, W, H, max_batch=B, max_candidates=args.max_candidates)
    det.set_cluster_sidecar(dists, rects, *side)
    det.upload(frames)
    det.enqueue(B, args.threshold)
    t.upload_scene(depth)
    per_frame = det.collect_clusters_depth(B, t, cap_total=args.cap_total)
    det.close()
    leaders, counts = [], []
    for (m, _, clusters, members) in per_frame:
        lead = cluster_leaders(clusters, members, m)
        leaders.append(m[lead])
        counts.append(len(lead))
    m = np.concatenate(leaders)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    poses = t.refine_poses(m, None, offsets, model_camera=cam, scene_camera=cam)
    P = pvc.make_params(cam, cam)
    kw = pvc.verify_kwargs(P)

    got = t.verify_poses(m, poses, None, offsets, **kw)
    wall = timed(lambda: t.verify_poses(m, poses, None, offsets, **kw), args.repeats)
    t.set_profiling(True)
    for _ in range(min(args.repeats, 200)):
        t.verify_poses(m, poses, None, offsets, **kw)
    ms_total, launches = t.kernel_times()["k_pose_verify"]
    t.set_profiling(False)

    used = sorted(set(int(i) for i in m["template_id"]))
    crops = [t.crop(k) if k in used else np.zeros((0, 0), np.uint16) for k in range(len(t))]
    with tempfile.TemporaryDirectory() as tmp:
        host = pvc.build_host(tmp, opt="-O3")
    on_host = host_jobs(host, crops, rects, depth, offsets, m, poses, P, POSE_VERIFY_DTYPE)
    want = on_host()
    assert got.tobytes() == want.tobytes(), "device and host records differ"
    cpu = timed(on_host, 5, warmup=1)
    t.close()

    points = got["n_model"].astype(np.int64)
    keep3, keep2 = keep_verified(got, 0.3), keep_verified(got, 0.2)
    dev_ms, cpu_ms = 1e3 * float(np.median(wall)), 1e3 * float(np.median(cpu))
    lines = ["pose verification of the cluster leaders of one %d-frame step, memoryChip2 (%d templates) at %d x %d, threshold %g (scripts/pose_verify_bench.py): "
             "recorded values, not thresholds" % (B, len(rects), W, H, args.threshold),
             "jobs: %d leaders (%.1f per frame, min %d, max %d); model points per job %d .. %d (median %d); voxel_mm %.1f, roi_margin %d"
             % (len(m), np.mean(counts), min(counts), max(counts), points.min(), points.max(), int(np.median(points)), P["voxel_mm"], P["roi_margin"]),
             "records: statuses %s (none, ok, empty, grid too large); cells per job median %d, max %d; scene pixels that marked a voxel, median %d; rate median %.3f; "
             "kept at 0.3: %d, at 0.2: %d" % (np.bincount(got["status"], minlength=4).tolist(), int(np.median(got["cells"])), int(got["cells"].max()),
                                             int(np.median(got["n_scene"])), float(np.median(got["rate"])), int(keep3.sum()), int(keep2.sum())),
             "",
             "device, verify_poses with the scene resident (job upload, one launch, read-back, one synchronisation), %d calls after 3 warm-up calls:" % args.repeats,
             "    %s" % spread(wall),
             "    k_pose_verify alone, event pairs in a loop of its own: %.3f ms per launch (%d launches)" % (ms_total / max(launches, 1), launches),
             "host, the same header on one core (g++ -O3 -ffp-contract=off), the same jobs, 5 runs after 1:",
             "    %s" % spread(cpu),
             "device records equal the host's, byte for byte",
             "",
             "ratio of the medians, one core / device call: %.1f (%.1f us against %.1f us per job)" % (cpu_ms / dev_ms, 1e3 * cpu_ms / len(m), 1e3 * dev_ms / len(m))]
    if cpu_ms <= dev_ms:
        lines.append("the device call is NOT faster than the one-core header for this job count")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
