"""Host cost of the device-resident path through the Python binding: the wall time of Detector.export_clusters(out=...) followed by
DepthTemplates.pose_chain(out=...) on one small resident frame set (tests/test_gpu_export_clusters.py's: 160 x 160, 80 templates, frames
A, Z, B of one enqueue that stays outstanding, depth-scored clusters).  Only the two calls are timed; the stream is synchronised after
each step, outside the timed region.  --detector PATH times another detector.py (a parent commit's) against the same library, for runs
that alternate the two: the file is loaded as a sibling module of the package's own.
Prints one line per run: the medians of the export call, the chain call and their sum in microseconds, with the sum's quartiles."""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detector", default=None, help="another detector.py to time in place of the package's")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    import torch
    from linemod_pose_estimation_amd import detector as D, synth
    from test_gpu_cluster_depth import make_crops
    if args.detector:
        spec = importlib.util.spec_from_file_location("linemod_pose_estimation_amd.detector_other", args.detector)
        D = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = D
        spec.loader.exec_module(D)
    S, THR, N_T, F = 160, 45.0, 80, 520.0
    bank = synth.make_bank(N_T, seed=91, size_range=(20.0, 36.0))
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(N_T) % 4) + rng.uniform(-0.005, 0.005, N_T)
    rects = np.stack([np.zeros(N_T), np.zeros(N_T), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    frames = [synth.make_scene(bank, S, S, seed=94)[0], [np.full((S, S, 3), 90, np.uint8), np.full((S, S), 800, np.uint16)],
              synth.make_scene(bank, S, S, seed=93, n_instances=1)[0]]
    dev = [[torch.from_numpy(np.ascontiguousarray(fr[0])).cuda(), torch.from_numpy(np.ascontiguousarray(fr[1]).view(np.int16)).cuda()] for fr in frames]
    det = D.Detector(bank, S, S, max_batch=3, max_candidates=1 << 17)
    det.set_cluster_sidecar(dists, rects, 10, 0.5, 0.1, 2)
    t = D.DepthTemplates.from_crops(make_crops(N_T, 31))
    cam = (F, F, S / 2.0, S / 2.0)
    kw = dict(rects=rects, model_camera=cam, scene_camera=cam, max_dist_mm=20.0, max_iterations=4, min_pairs=3, search_radius=1, voxel_mm=8.0, roi_margin=4)
    stream = torch.cuda.current_stream()
    det.upload_device(dev)
    det.enqueue(3, THR)
    t.upload_scene_device([d[1] for d in dev])
    res = poses = None
    export_ns, chain_ns = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter_ns()
        res = det.export_clusters(3, templates=t, max_large_frames=1, out=res)
        t1 = time.perf_counter_ns()
        poses = t.pose_chain(res, 0.3, out=poses, **kw)
        t2 = time.perf_counter_ns()
        stream.synchronize()
        if step >= args.warmup:
            export_ns.append(t1 - t0)
            chain_ns.append(t2 - t1)
    hdr = poses.to_host()[0]
    both = np.asarray(export_ns) + np.asarray(chain_ns)
    q = np.percentile(both, [25, 50, 75]) / 1e3
    print("%-6s steps %d  export %.2f us  chain %.2f us  both %.2f us (quartiles %.2f .. %.2f)  slots %d kept %d"
          % (args.label, args.steps, np.median(export_ns) / 1e3, np.median(chain_ns) / 1e3, q[1], q[0], q[2], hdr[0], hdr[4]), flush=True)
    det.release()
    t.close()
    det.close()


if __name__ == "__main__":
    main()
