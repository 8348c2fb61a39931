#!/usr/bin/env python3
"""What leaving the final matches in device memory costs or saves (lmx_ctx_export_matches_on) on the default workload as bench.py builds
it: 640x480 RGB-D, 3000 templates, threshold 92, 64 frames per step, frames fed from device tensors every step (three batches rotate).
  export   upload_device; enqueue; export_matches(out=the same buffers); a trivial torch consumer on the stream (the sum of the delivered
           similarities); release
  collect  upload_device; enqueue; collect; the match list re-uploaded as one tensor; the same consumer on it
Both legs are timed with the host clock around one whole step, which ends in a synchronisation of the consumer's stream in either leg (one
step in flight: latency of a step, not the pipelined rate).  The legs ALTERNATE step by step in one process; reported are the median,
the quartiles and the extremes of each leg and the median of the per-pair differences.  Before timing, the two legs' match lists are
compared bit for bit.  Then the device memory the export holds: free memory before and after a context's first export, next to what the
library itself allocates and to what the first collect_clusters of another context takes.
Needs a GPU.  usage: device_output_bench.py [--repeats 60] [--max-large-frames 0] [--export-first] [--out profiles/device_output.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload's constants)

W, H, B, THR, N_TEMPLATES = bench.WIDTH, bench.HEIGHT, 64, bench.THRESHOLD, bench.TEMPLATES_PER_GPU


def spread(ts):
    ts = 1e3 * np.asarray(ts)
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "median %.3f ms (quartiles %.3f .. %.3f, min %.3f, max %.3f)" % (q[2], q[1], q[3], q[0], q[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--max-large-frames", type=int, default=0)
    ap.add_argument("--export-first", action="store_true", help="the export is the first call of the process that runs the finalise kernel (memory figures)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from linemod_pose_estimation_amd import Detector, synth
    if not torch.cuda.is_available():
        raise SystemExit("device_output_bench.py needs a GPU")
    bank = synth.make_bank(N_TEMPLATES, modalities=("ColorGradient", "DepthNormal"), T=(5, 8), seed=20250215)
    frames = [synth.make_scene(bank, W, H, seed=3000 + f, row_pad=0, texture=0.6)[0] for f in range(B)]
    frames = [[np.ascontiguousarray(s) for s in fr] for fr in frames]
    perms = [np.random.default_rng(s).permutation(B) for s in (1, 2, 3)]
    dev = [Detector.prepare_device_batch([[torch.from_numpy(s.view(np.int16) if s.dtype == np.uint16 else s).cuda() for s in frames[i]] for i in p]) for p in perms]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()

    def first_collect_clusters():
        """what a context's first collect_clusters takes (its chain runs the same finalise kernel on a stream of its own)"""
        other = Detector(bank, W, H, max_batch=B, overlap=True)
        other.set_cluster_sidecar(0.5 + 0.1 * (np.arange(N_TEMPLATES) % 4), np.tile(np.array([0, 0, 32, 32], np.int32), (N_TEMPLATES, 1)), 10, 0.5, 0.1, 2)
        other.upload_device(dev[0])
        other.enqueue(B, THR)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        other.collect_clusters(B)
        torch.cuda.synchronize()
        took = before - torch.cuda.mem_get_info()[0]
        other.close()
        torch.cuda.synchronize()
        return took

    collect_took = None if args.export_first else first_collect_clusters()
    free0 = torch.cuda.mem_get_info()[0]
    det = Detector(bank, W, H, max_batch=B, overlap=True)
    det.upload_device(dev[0])
    det.enqueue(B, THR)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    buf = det.export_matches(B, max_large_frames=args.max_large_frames)
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    out_bytes = sum(t.numel() * t.element_size() for t in buf._backing.values())
    det.release()
    if collect_took is None:
        collect_took = first_collect_clusters()

    def consume(matches, n):
        return matches[:n, 2].view(torch.float32).sum()

    def export_leg(i):
        det.upload_device(dev[i % 3])
        det.enqueue(B, THR)
        res = det.export_matches(B, max_large_frames=args.max_large_frames, out=buf)
        # the consumer never learns the count on the host: it reads the whole array's delivered part through the header on the device
        n = res.header[2].clamp(max=res.caps[0])
        idx = torch.arange(res.caps[0], device=res.matches.device)
        total = torch.where(idx < n, res.similarity, torch.zeros((), device=idx.device)).sum()
        det.release()
        stream.synchronize()
        return res, total

    def collect_leg(i):
        det.upload_device(dev[i % 3])
        det.enqueue(B, THR)
        per_frame = det.collect(B)
        flat = np.concatenate(per_frame)
        t = torch.from_numpy(flat.view(np.int32).reshape(-1, 5)).cuda()
        total = consume(t, len(flat))
        stream.synchronize()
        return per_frame, total

    # the same lists, bit for bit
    res, tot_e = export_leg(0)
    per_frame, tot_c = collect_leg(0)
    host = res.to_host()
    hdr = res.header.cpu().numpy()
    n_delivered = 0
    for f in range(B):
        if host[f] is not None:
            assert host[f][0].tobytes() == per_frame[f].tobytes(), f
            n_delivered += 1
    assert n_delivered > 0
    n_matches = [len(m) for m in per_frame]
    for i in range(1, 4):
        export_leg(i)
        collect_leg(i)
    te, tc = [], []
    for i in range(args.repeats):
        t0 = time.perf_counter()
        export_leg(i)
        t1 = time.perf_counter()
        collect_leg(i)
        t2 = time.perf_counter()
        te.append(t1 - t0)
        tc.append(t2 - t1)
    det.close()
    diff = 1e3 * (np.asarray(tc) - np.asarray(te))
    iqr = 1e3 * (np.percentile(tc, 75) - np.percentile(tc, 25))
    lines = ["# scripts/device_output_bench.py  %s  %s  device %s" % (time.strftime("%Y-%m-%d %H:%M"), platform.node(), torch.cuda.get_device_name(0)),
             "default workload: %dx%d RGB-D, %d templates, threshold %g, %d frames per step from device tensors, three device lanes; one step in flight, "
             "%d alternating repeats" % (W, H, N_TEMPLATES, THR, B, args.repeats),
             "%.1f matches per frame (min %d, max %d), %d raw records per step; the export delivered %d of %d frames with max_large_frames=%d (header flags %d); "
             "delivered lists equal collect's bit for bit" % (np.mean(n_matches), min(n_matches), max(n_matches), hdr[6], n_delivered, B, args.max_large_frames, hdr[1]),
             "    export   upload_device, enqueue, export_matches, consumer on the stream, release, stream sync        %s" % spread(te),
             "    collect  upload_device, enqueue, collect, re-upload of the list, consumer, stream sync              %s" % spread(tc),
             "    collect - export, pair by pair: median %.3f ms (quartiles %.3f .. %.3f); the collect leg's own interquartile range is %.3f ms"
             % (np.median(diff), np.percentile(diff, 25), np.percentile(diff, 75), iqr),
             "device memory (hipMemGetInfo): the context before its first export %.1f MB; the first export took %.1f MB more.  Of that the library allocates %.1f MB "
             "(rows and chain scratch for %d frames) + %.1f MB (large-frame workspace for %d frames) and torch %.1f MB of outputs at the default capacities; "
             "the rest is the runtime's and torch's.  The HIP runtime sets memory aside for a hardware queue when a kernel with private memory (the finalise "
             "kernel: 1112 bytes per lane) first runs on it, and maps streams to queues as it sees fit: the first collect_clusters of another context, %s this "
             "export, took %.1f MB"
             % ((free0 - free1) / 1e6, (free1 - free2) / 1e6, B * 2048 * (20 + 48 + 4 + 32) / 1e6, B, min(args.max_large_frames, B) * 2457600 / 1e6,
                args.max_large_frames, out_bytes / 1e6, "after" if args.export_first else "before", collect_took / 1e6),
             "sums of the similarities, export / collect leg: %.3f / %.3f" % (float(tot_e), float(tot_c))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
