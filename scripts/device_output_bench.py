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
With --score depth|normal the same for the scored clusters (lmx_ctx_export_clusters_on), legs alternating in the same way:
  E        upload_device; enqueue; upload_scene_device; export_clusters(out=the same buffers); the consumer on the stream; release
  P        what the library offered before: upload_device; enqueue; upload_scene_device; collect_clusters_depth (or _depth_normal); matches,
           diffs (ndiffs), clusters and members re-uploaded as tensors; the same consumer
then the device time of the crop walk per launch (DepthTemplates.set_profiling): the one-workgroup-per-record kernel of the collect against
the persistent kernel of the export at several grids, on the default workload's record list and on a longer one (a lower threshold); and the
memory the first scored export takes.  The default bank has no mesh, so the depth templates are synthetic crops: a tilted plane of each
template's rect size.
Needs a GPU.  usage: device_output_bench.py [--repeats 60] [--max-large-frames 0] [--export-first] [--score depth|normal] [--out FILE]"""
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


def scored(args, torch, bank, frames, perms, dev):
    from linemod_pose_estimation_amd import DepthTemplates, Detector
    normal = args.score == "normal"
    stream = torch.cuda.current_stream()
    scene = [[torch.from_numpy(frames[i][1].view(np.int16)).cuda() for i in p] for p in perms]
    sizes = [(int(m["width"]), int(m["height"])) for m in bank.meta["obj"]]
    rects = np.asarray([(0, 0, w, h) for w, h in sizes], np.int32)
    dists = 0.5 + 0.1 * (np.arange(N_TEMPLATES) % 4)
    yy, xx = np.mgrid[0:max(h for _, h in sizes), 0:max(w for w, _ in sizes)]
    t = DepthTemplates.from_crops([(800 + 2 * xx[:h, :w] + 3 * yy[:h, :w]).astype(np.uint16) for w, h in sizes])
    if normal:
        t.enable_normals(570.0, 570.0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    det = Detector(bank, W, H, max_batch=B, overlap=True)
    det.set_cluster_sidecar(dists, rects, 10, 0.5, 0.1, 2)
    state = {"thr": THR, "buf": None}

    def front(i):
        det.upload_device(dev[i % 3])
        det.enqueue(B, state["thr"])
        t.upload_scene_device(scene[i % 3])

    def consume(matches, n):
        return matches[:n, 2].view(torch.float32).sum()

    def e_leg(i):
        front(i)
        res = det.export_clusters(B, templates=t, normals=normal, max_large_frames=args.max_large_frames, out=state["buf"])
        state["buf"] = res
        n = res.header[2].clamp(max=res.caps[0])
        idx = torch.arange(res.caps[0], device=res.matches.device)
        total = torch.where(idx < n, res.similarity, torch.zeros((), device=idx.device)).sum()
        det.release()
        stream.synchronize()
        return res, total

    def p_leg(i):
        front(i)
        got = det.collect_clusters_depth_normal(B, t) if normal else det.collect_clusters_depth(B, t)
        flat = np.concatenate([g[0] for g in got])
        up = [torch.from_numpy(flat.view(np.int32).reshape(-1, 5)).cuda()]
        for k in range(1, len(got[0]) - 1):                   # diffs, (ndiffs,) clusters
            a = np.concatenate([g[k] for g in got])
            up.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)).cuda())
        n_mem = sum(int(g[-2]["member_count"].sum()) for g in got)
        up.append(torch.from_numpy(got[0][-1][:max(n_mem, 1)]).cuda())
        total = consume(up[0], len(flat))
        stream.synchronize()
        return got, total

    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    res, tot_e = e_leg(0)
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    got, tot_p = p_leg(0)
    host, hdr = res.to_host(), res.header.cpu().numpy()
    n_delivered = 0
    for f in range(B):
        if host[f] is not None:
            n_delivered += 1
            for a, b in zip((host[f][0], host[f][1], host[f][2] if normal else None, host[f][3]["score"]), (got[f][0], got[f][1], got[f][2] if normal else None, got[f][-2]["score"])):
                assert a is None or a.tobytes() == b.tobytes(), f
    assert n_delivered > 0
    n_clusters = sum(len(g[-2]) for g in got)
    for i in range(1, 4):
        e_leg(i)
        p_leg(i)
    te, tp = [], []
    for i in range(args.repeats):
        t0 = time.perf_counter()
        e_leg(i)
        t1 = time.perf_counter()
        p_leg(i)
        t2 = time.perf_counter()
        te.append(t1 - t0)
        tp.append(t2 - t1)
    diff = 1e3 * (np.asarray(tp) - np.asarray(te))
    iqr = 1e3 * (np.percentile(tp, 75) - np.percentile(tp, 25))
    # the walk alone, per launch, three rounds of each form so that the spread shows
    old_name = "k_verify_diff_records" if normal else "k_depth_diff_records"
    grids = [cus, 2 * cus, 4 * cus, 8 * cus]
    table = []
    for thr in (THR, args.walk_threshold):
        state["thr"] = thr
        rows = {}
        for rnd in range(3):
            for form in ["one workgroup per record"] + grids:
                if form in grids:
                    t.debug_walk_grid(form)
                leg, name = (e_leg, "k_walk_records_dev") if form in grids else (p_leg, old_name)
                leg(0)
                t.set_profiling(True)
                for i in range(20):
                    leg(i)
                ms, n = t.kernel_times()[name]
                t.set_profiling(False)
                rows.setdefault(form, []).append(1e3 * ms / max(n, 1))
        t.debug_walk_grid(0)
        e_leg(0)
        table.append((thr, int(state["buf"].header[6]), rows))
    det.close()
    t.close()
    lines = ["# scripts/device_output_bench.py --score %s  %s  %s  device %s, %d compute units" % (args.score, time.strftime("%Y-%m-%d %H:%M"), platform.node(), torch.cuda.get_device_name(0), cus),
             "default workload: %dx%d RGB-D, %d templates, threshold %g, %d frames per step from device tensors; one step in flight, %d alternating repeats.  Depth "
             "templates: synthetic crops (a tilted plane of each template's rect size; the default bank has no mesh)" % (W, H, N_TEMPLATES, THR, B, args.repeats),
             "%d raw records per step, %d clusters; the export delivered %d of %d frames with max_large_frames=%d (header flags %d); delivered matches, diffs%s and "
             "cluster scores equal the collect's bit for bit" % (hdr[6], n_clusters, n_delivered, B, args.max_large_frames, hdr[1], ", ndiffs" if normal else ""),
             "    E  upload_device, enqueue, upload_scene_device, export_clusters, consumer on the stream, release, stream sync                 %s" % spread(te),
             "    P  upload_device, enqueue, upload_scene_device, collect_clusters_%s, re-upload of matches, diffs, clusters, members, consumer   %s"
             % ("depth_normal" if normal else "depth", spread(tp)),
             "    P - E, pair by pair: median %.3f ms (quartiles %.3f .. %.3f); leg P's own interquartile range is %.3f ms" % (np.median(diff), np.percentile(diff, 25), np.percentile(diff, 75), iqr),
             "the crop walk alone, device time per launch in microseconds (event pairs, 20 launches per figure, three rounds):"]
    for thr, n_rec, rows in table:
        lines.append("  threshold %g, %d raw records per step" % (thr, n_rec))
        for form, v in rows.items():
            what = "%-28s" % (form if isinstance(form, str) else "persistent, %d workgroups (%d per CU)" % (form, form // cus))
            lines.append("    %-44s %s   median %.2f" % (what, "  ".join("%.2f" % x for x in v), float(np.median(v))))
    lines.append("device memory (hipMemGetInfo): the first scored export of the context took %.1f MB; of that the library allocates %.1f MB per-record results "
                 "(%d records of capacity x %d B) and %.1f MB of rows for %d frames, torch the outputs" %
                 ((free1 - free2) / 1e6, 16384 * B * (32 if normal else 16) / 1e6, 16384 * B, 32 if normal else 16, B * 2048 * 48 * (2 if normal else 1) / 1e6, B))
    lines.append("sums of the similarities, E / P leg: %.3f / %.3f" % (float(tot_e), float(tot_p)))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--max-large-frames", type=int, default=0)
    ap.add_argument("--export-first", action="store_true", help="the export is the first call of the process that runs the finalise kernel (memory figures)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--score", choices=("depth", "normal"), default=None, help="measure export_clusters against collect_clusters_depth / _depth_normal instead")
    ap.add_argument("--walk-threshold", type=float, default=86.0, help="--score: the lower threshold of the walk kernels' second, longer record list")
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
    if args.score:
        text = scored(args, torch, bank, frames, perms, dev)
        print(text, end="")
        if args.out:
            with open(args.out, "a") as f:
                f.write(text)
        return
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
