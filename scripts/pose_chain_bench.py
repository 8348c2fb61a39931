#!/usr/bin/env python3
"""The pose stages behind an export, host-staged against on the device (DepthTemplates.pose_chain = lmx_pose_chain_on), on the workload of
profiles/pose_verify.txt: the 2652-view memoryChip2 bank at 640x480, one 64-frame step, the depth-scored clusters of
Detector.export_clusters (the bank, renders and frames of scripts/pose_verify_bench.py).  One enqueue stays outstanding and the scene
resident; each step exports again, since an export consumes nothing:
  staged   export_clusters -> to_host() -> cluster_leaders per frame -> refine_poses -> verify_poses -> keep_verified
  chain    export_clusters -> pose_chain -> one synchronisation of the stream
The legs alternate, step by step, on the same process and box; wall time per step from the host clock, medians with quartiles and
extremes.  The chain's results must equal the staged ones byte for byte before anything is timed.  Then the device time of the kernels
from the object's event pairs (set_profiling), in blocks of steps so that the blocks' spread is recorded next to the means:
k_pose_refine + k_pose_verify of the staged leg against k_pose_refine_clusters + k_pose_verify_clusters of the chain, for the same jobs.
The chain's grid is cap_clusters workgroups, of which those at or above the live count leave at once: every figure is taken for each
--cap-clusters value.  These are recorded values, not thresholds.  Needs a GPU.
--schedule: every leg refines under that schedule (DepthTemplates.set_refine_schedule); the byte-for-byte check is the same.
--plane: every leg refines with those point_shift values, one per stage (DepthTemplates.set_refine_plane, after enable_normals with the
scene camera's focal lengths); "--schedule 1:5:10:1 --plane 8" is the point-to-plane metric at 5 iterations.
usage: pose_chain_bench.py [--threshold 80] [--repeats 40] [--cap-clusters 4096 512] [--schedule S] [--plane K[,K..]] [--out profiles/pose_chain.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480
B = 64
KEEP = 0.3


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, default=80.0)
    ap.add_argument("--repeats", type=int, default=40, help="steps per leg in the timed window")
    ap.add_argument("--blocks", type=int, default=5, help="blocks of --block-steps steps for the kernels' device time")
    ap.add_argument("--block-steps", type=int, default=10)
    ap.add_argument("--cap-clusters", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--max-candidates", type=int, default=1 << 19)
    ap.add_argument("--schedule", default=None, help="stride:iterations:max_dist:radius,...: the refinement schedule every leg runs under")
    ap.add_argument("--plane", default=None, help="point_shift per stage, comma-separated: -1 point-to-point, 0..20 point-to-plane")
    ap.add_argument("--scene-filter", action="store_true", help="the pose stages read the filtered scene (DepthTemplates.set_scene_filter, the defaults)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_chain.txt"))
    args = ap.parse_args()
    import torch
    import pose_verify_cases as pvc
    from linemod_pose_estimation_amd import DepthTemplates, Detector, cluster_leaders, keep_verified, meshsynth as ms

    F = ms.ENSENSO["fx"]
    cam = (F, F, W / 2.0, H / 2.0)
    side = (8, ms.ENSENSO["radius_min"], ms.ENSENSO["radius_step"], 2)
    bank, rects, dists, view_of = ms.load_bank("memoryChip2")
    chip, cpu_mesh, grid = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary"), ms.view_grid()
    t = DepthTemplates.from_mesh(chip, [grid[int(v)] for v in view_of], W, H, F, F)
    if args.schedule:
        import pose_refine_staged_cases as psc
        t.set_refine_schedule(psc.parse_schedule(args.schedule))
    if args.plane:
        t.enable_normals(F, F)
        t.set_refine_plane([int(v) for v in args.plane.split(",")])
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
    lines = ["the pose stages behind one 64-frame export, memoryChip2 (%d templates) at %d x %d, threshold %g (scripts/pose_chain_bench.py): recorded values, not thresholds"
             % (len(rects), W, H, args.threshold)]
    if args.schedule:
        lines.append("refinement schedule of every leg: [%s]" % args.schedule)
    if args.plane:
        lines.append("point_shift of every leg's stages: [%s]" % args.plane)
    if args.scene_filter:
        lines.append("scene filter set (radius 3, k 15, stddev_mul 1.0): every leg's pose stages read the filtered scene")

    for cap in args.cap_clusters:
        state = {"res": None, "poses": None}

        def export():
            state["res"] = det.export_clusters(B, templates=t, max_large_frames=B, cap_clusters=cap, stream=stream, out=state["res"])
            return state["res"]

        def staged():
            host = export().to_host()
            lead, counts = [], []
            for fr in host:
                m, _, _, cl, _, mem = fr
                k = cluster_leaders(cl, mem, m) if len(cl) else np.zeros(0, np.int64)
                lead.append(m[k])
                counts.append(len(k))
            m = np.concatenate(lead)
            offs = np.concatenate([[0], np.cumsum(counts)])
            p = t.refine_poses(m, None, offs, model_camera=cam, scene_camera=cam)
            c = t.verify_poses(m, p, None, offs, **vkw)
            return m, p, c, keep_verified(c, KEEP)

        def chain():
            state["poses"] = t.pose_chain(export(), KEEP, out=state["poses"], **vkw)
            stream.synchronize()
            return state["poses"]

        m, p, c, keep = staged()
        hdr, leaders, gp, gc, gkeep = chain().to_host()
        info = state["res"].frame_info.cpu().numpy()
        assert (info[:, 6] == 0).all() and hdr[0] == len(m) and hdr[1] == 0, (hdr, info[:, 6])
        all_m = state["res"].to_host()
        flat = np.concatenate([fr[0] for fr in all_m])
        assert flat[leaders].tobytes() == m.tobytes() and gp.tobytes() == p.tobytes() and gc.tobytes() == c.tobytes() and np.array_equal(gkeep, keep), "the chain and the staged path differ"

        for _ in range(3):
            staged()
            chain()
        wall = {"staged": [], "chain": []}
        for _ in range(args.repeats):
            for name, fn in (("staged", staged), ("chain", chain)):
                t0 = time.perf_counter()
                fn()
                wall[name].append(time.perf_counter() - t0)
        # the export alone, for what both legs share
        only = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            export()
            stream.synchronize()
            only.append(time.perf_counter() - t0)

        per_block = {"staged": [], "chain": []}
        for _ in range(args.blocks):
            for name, fn, kernels in (("staged", staged, ("k_pose_refine", "k_pose_verify")), ("chain", chain, ("k_pose_refine_clusters", "k_pose_verify_clusters"))):
                t.set_profiling(True)
                for _ in range(args.block_steps):
                    fn()
                times = t.kernel_times()
                t.set_profiling(False)
                assert all(times[k][1] == args.block_steps for k in kernels), times
                per_block[name].append([times[k][0] / args.block_steps for k in kernels])
        dev = {k: np.asarray(v) for k, v in per_block.items()}

        def blocks(a):
            return "mean %.3f ms (blocks %.3f .. %.3f)" % (a.mean(), a.min(), a.max())
        s, ch = dev["staged"], dev["chain"]
        lines += ["",
                  "cap_clusters %d (the chain's grid): %d live clusters of %d frames, statuses of the poses %s, of the checks %s, kept at %.1f: %d"
                  % (cap, len(m), B, np.bincount(p["status"], minlength=5).tolist(), np.bincount(c["status"], minlength=4).tolist(), KEEP, int(keep.sum())),
                  "the chain's leaders, poses, checks and keep decisions equal the staged path's, byte for byte",
                  "wall time per step, %d steps per leg, the legs alternating, after 3 warm-up steps each:" % args.repeats,
                  "    staged  export -> to_host -> cluster_leaders -> refine_poses -> verify_poses -> keep_verified: %s" % spread(wall["staged"]),
                  "    chain   export -> pose_chain -> one synchronisation:                                           %s" % spread(wall["chain"]),
                  "    export -> one synchronisation alone:                                                          %s" % spread(only),
                  "device time of the kernels per step, event pairs, %d blocks of %d steps per leg, the legs alternating:" % (args.blocks, args.block_steps),
                  "    k_pose_refine           %s    k_pose_verify           %s    sum %s" % (blocks(s[:, 0]), blocks(s[:, 1]), blocks(s.sum(1))),
                  "    k_pose_refine_clusters  %s    k_pose_verify_clusters  %s    sum %s" % (blocks(ch[:, 0]), blocks(ch[:, 1]), blocks(ch.sum(1))),
                  "    difference of the sums' means, chain - staged: %+.3f ms; spread of the staged sum over its blocks: %.3f ms, of the chain's: %.3f ms"
                  % (ch.sum(1).mean() - s.sum(1).mean(), s.sum(1).max() - s.sum(1).min(), ch.sum(1).max() - ch.sum(1).min())]
    det.release()
    det.close()
    t.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
