#!/usr/bin/env python3
"""What the rough pose stage costs: DepthTemplates.rough_pose_chain (lmx_rough_pose_chain_on: orientation groups, mean view, the mesh
rendered again, then both pose stages) against DepthTemplates.pose_chain (the leader's stored crop through both pose stages) on the same
exported clusters, on the workload of profiles/pose_chain.txt: the 2652-view memoryChip2 bank at 640x480, one 64-frame step, the
depth-scored clusters of Detector.export_clusters.  One enqueue stays outstanding and the scene resident; one export feeds both calls.
Device time per call from an event pair on the caller's stream around it (the call's kernels run on the object's stream between the two
waits the call queues), the two calls alternating, medians with quartiles and extremes.  These are recorded values, not thresholds.
--kernels N: nothing is timed; N calls of each are made for a kernel trace taken from outside (rocprofv3 --kernel-trace --stats).
Needs a GPU.
--schedule: every leg refines under that schedule (DepthTemplates.set_refine_schedule).
usage: rough_pose_bench.py [--threshold 80] [--repeats 40] [--cap-clusters 512] [--window 320] [--degrees 10] [--schedule S] [--out profiles/rough_pose.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480
B = 64
KEEP = 0.3


def spread(ms):
    q = np.percentile(np.asarray(ms), [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, default=80.0)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--cap-clusters", type=int, default=512)
    ap.add_argument("--window", type=int, default=320)
    ap.add_argument("--degrees", type=float, default=10.0)
    ap.add_argument("--max-candidates", type=int, default=1 << 19)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--schedule", default=None, help="stride:iterations:max_dist:radius,...: the refinement schedule every leg runs under")
    ap.add_argument("--scene-filter", action="store_true", help="the pose stages read the filtered scene (DepthTemplates.set_scene_filter, the defaults)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rough_pose.txt"))
    args = ap.parse_args()
    import torch
    import pose_verify_cases as pvc
    from linemod_pose_estimation_amd import DepthTemplates, Detector, RoughModel, meshsynth as ms

    F = ms.ENSENSO["fx"]
    cam = (F, F, W / 2.0, H / 2.0)
    side = (8, ms.ENSENSO["radius_min"], ms.ENSENSO["radius_step"], 2)
    bank, rects, dists, view_of = ms.load_bank("memoryChip2")
    chip, cpu_mesh, grid = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary"), ms.view_grid()
    views = [grid[int(v)] for v in view_of]
    t = DepthTemplates.from_mesh(chip, views, W, H, F, F)
    if args.schedule:
        import pose_refine_staged_cases as psc
        t.set_refine_schedule(psc.parse_schedule(args.schedule))
    model = RoughModel(chip, views, W, H, F, F, ori_dists=dists, cap_slots=args.cap_clusters, max_window=(args.window, args.window))
    if args.scene_filter:
        t.set_scene_filter(camera=cam)
    distinct = [ms.make_scene(chip, grid, seed=7000 + f, n_instances=3, other_tri=cpu_mesh, n_other=2)[0] for f in range(16)]
    frames = [distinct[f % len(distinct)] for f in range(B)]
    depth = [np.ascontiguousarray(fr[1]) for fr in frames]
    det = Detector(bank, W, H, max_batch=B, max_candidates=args.max_candidates)
    det.set_cluster_sidecar(dists, rects, *side)
    det.upload(frames)
    det.enqueue(B, args.threshold)
    t.upload_scene(depth)
    vkw = pvc.verify_kwargs(pvc.make_params(cam, cam))
    stream = torch.cuda.Stream()
    res = det.export_clusters(B, templates=t, max_large_frames=B, cap_clusters=args.cap_clusters, stream=stream)
    state = {"leader": None, "rough": None}

    def leader():
        state["leader"] = t.pose_chain(res, KEEP, out=state["leader"], **vkw)

    def rough():
        state["rough"] = t.rough_pose_chain(res, model, KEEP, threshold_deg=args.degrees, out=state["rough"], **vkw)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    with torch.cuda.stream(stream):
        leader()
        rough()
    lh, _, lp, lc, lk = state["leader"].to_host()
    rh, rr, _, rp, rc, rk = state["rough"].to_host()
    info = res.frame_info.cpu().numpy()
    assert (info[:, 6] == 0).all() and lh[0] == rh[0] > 0, (lh, rh, info[:, 6])
    if args.kernels:
        with torch.cuda.stream(stream):
            for _ in range(args.kernels):
                leader()
                rough()
        stream.synchronize()
        print("%d calls of each made" % (args.kernels + 1))
        det.release()
        return
    for _ in range(3):
        timed(leader)
        timed(rough)
    ms_of = {"leader": [], "rough": []}
    for _ in range(args.repeats):
        ms_of["leader"].append(timed(leader))
        ms_of["rough"].append(timed(rough))
    lines = ["the rough pose stage behind one 64-frame export, memoryChip2 (%d templates, %d triangles) at %d x %d, threshold %g (scripts/rough_pose_bench.py): recorded values, "
             "not thresholds" % (len(rects), len(chip), W, H, args.threshold)] + (["refinement schedule of every leg: [%s]" % args.schedule] if args.schedule else []) + ["",
             "cap_clusters %d (every kernel's grid), orientation threshold %g degrees, window %d x %d, the model object holds %.1f MB"
             % (args.cap_clusters, args.degrees, args.window, args.window, model.device_bytes() / 1e6),
             "%d live clusters of %d frames; members per cluster %d .. %d (mean %.1f), groups per cluster %d .. %d (mean %.1f), members of the winning group mean %.1f"
             % (rh[0], B, rr["n_members"].min(), rr["n_members"].max(), rr["n_members"].mean(), rr["n_groups"].min(), rr["n_groups"].max(), rr["n_groups"].mean(),
                rr["n_group_members"].mean()),
             "rough statuses (none, ok, too many groups, degenerate, invalid view, window too large, empty) %s; covered pixels of a render mean %.0f"
             % (np.bincount(rr["status"], minlength=7).tolist(), rr["n_model"][rr["status"] == 1].mean() if (rr["status"] == 1).any() else 0.0),
             "pose_chain:        statuses of the poses %s, of the checks %s, kept at %.1f: %d; model points per job mean %.0f"
             % (np.bincount(lp["status"], minlength=5).tolist(), np.bincount(lc["status"], minlength=4).tolist(), KEEP, int(lk.sum()), lp["n_model"].mean()),
             "rough_pose_chain:  statuses of the poses %s, of the checks %s, kept at %.1f: %d; model points per job mean %.0f"
             % (np.bincount(rp["status"], minlength=5).tolist(), np.bincount(rc["status"], minlength=4).tolist(), KEEP, int(rk.sum()), rp["n_model"].mean()),
             "device time per call, an event pair on the caller's stream around it, %d calls each, alternating, after 3 warm-up calls each:" % args.repeats,
             "    pose_chain (leader's stored crop):                 %s" % spread(ms_of["leader"]),
             "    rough_pose_chain (groups, mean view, re-render):   %s" % spread(ms_of["rough"])]
    det.release()
    det.close()
    model.close()
    t.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
