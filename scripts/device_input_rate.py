#!/usr/bin/env python3
"""What frames that already live in device memory cost to match (lmx_ctx_upload_device) on the default workload as bench.py builds it:
640x480 RGB-D, 3000 templates, threshold 92, 64 frames per step, three device lanes.  One process, one box, the legs alternated
(--rounds of each), every line the median of its rounds with the spread next to it:
  (a) resident   frames uploaded once, no upload in the timed steps (bench.py's headline)
  (b) device     upload_device of a fresh batch of device tensors every step (three batches rotate; descriptors built once)
  (c) pageable   upload of fresh pageable host frames every step (bench.py's host_frames)
and the device time per step of the pre-processing stage ("k_pre", HIP events around its launches, one step in flight) on ONE input --
64 raw 752x480 MONO8 frames + float-metre depth, blurred and cropped to 640x480 -- through upload_device (k_ingest, frames in device
memory) and through upload_raw (k_pre_color / k_pre_depth, behind the host copy and the DMA, which the events do not cover); then the
same stage for feed (b)'s plain copy, and the host time of one upload_device call.
Needs a GPU.  usage: device_input_rate.py [--rounds 3] [--steps 60]"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (timing helpers: run_pipelined, secondary_line; the workload's constants)

W, H, B, THR, N_TEMPLATES = bench.WIDTH, bench.HEIGHT, 64, bench.THRESHOLD, bench.TEMPLATES_PER_GPU
RAW_W, CROP_X = 752, 56


def med(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def spread(xs):
    return "%.4g .. %.4g" % (min(xs), max(xs))


def to_device(torch, frames):
    """numpy frames -> torch tensors on the GPU; uint16 as int16 (its bit pattern)."""
    return [[torch.from_numpy(s.view(np.int16) if s.dtype == np.uint16 else s).cuda() for s in fr] for fr in frames]


def k_pre_ms(det, upload, steps=3):
    det.set_profiling("k_pre")
    det.reset_profiling()
    for _ in range(steps):
        upload()
        det.enqueue(B, THR)
        det.collect(B)
    ms, launches = det.kernel_times()["k_pre"]
    det.set_profiling(False)
    return ms / steps, launches // steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    import torch
    from linemod_pose_estimation_amd import Detector, synth
    if not torch.cuda.is_available():
        raise SystemExit("device_input_rate.py needs a GPU")
    bank = synth.make_bank(N_TEMPLATES, modalities=("ColorGradient", "DepthNormal"), T=(5, 8), seed=20250215)
    frames = [synth.make_scene(bank, W, H, seed=3000 + f, row_pad=0, texture=0.6)[0] for f in range(B)]
    frames = [[np.ascontiguousarray(s) for s in fr] for fr in frames]
    perms = [np.random.default_rng(s).permutation(B) for s in (1, 2, 3)]
    host_batches = [[[np.array(src, copy=True) for src in frames[i]] for i in p] for p in perms]
    host_prepared = [Detector.prepare_batch(b) for b in host_batches]
    dev_prepared = [Detector.prepare_device_batch(to_device(torch, b)) for b in host_batches]
    torch.cuda.synchronize()

    def up_device(det, i):
        det.upload_device(dev_prepared[i % len(dev_prepared)])

    # the raw camera input of the k_pre comparison: MONO8 752x480 (the scene's green channel, padded) + float metres
    raw = []
    for fr in frames:
        mono = np.ascontiguousarray(np.pad(fr[0][:, :, 1], ((0, 0), (CROP_X, RAW_W - W - CROP_X)), mode="edge"))
        z = np.ascontiguousarray(np.pad(fr[1], ((0, 0), (CROP_X, RAW_W - W - CROP_X)), mode="edge").astype(np.float32) / np.float32(1000.0))
        raw.append([mono, z])
    raw_host = Detector.prepare_batch(raw)
    raw_dev = Detector.prepare_device_batch(to_device(torch, raw))
    torch.cuda.synchronize()

    feeds = {"resident": [], "device": [], "pageable": []}
    matches = {}
    for r in range(args.rounds):
        order = ("resident", "device", "pageable") if r % 2 == 0 else ("pageable", "device", "resident")
        for feed in order:
            if feed == "resident":
                line = bench.secondary_line(torch, Detector, bank, host_batches[0], B, THR, args.steps)
            else:
                line = bench.secondary_line(torch, Detector, bank, None, B, THR, args.steps, uploads=up_device if feed == "device" else host_prepared)
            feeds[feed].append(line["value"] / B)            # steps/s
            matches[feed] = line["matches_per_frame"]
    pre = {"ingest": [], "k_pre": []}
    det = Detector(bank, W, H, max_batch=B, overlap=True)
    legs = {"ingest": lambda: det.upload_device(raw_dev, src_size=(RAW_W, H), crop_xy=(CROP_X, 0), blur3=True, mono=True, depth_float_m=True),
            "k_pre": lambda: det.upload_raw(raw_host, (RAW_W, H), (CROP_X, 0), blur3=True, mono=True, depth_float_m=True)}
    for leg in legs.values():      # warm both
        leg()
        det.enqueue(B, THR)
        det.collect(B)
    launches = {}
    for r in range(max(args.rounds, 3)):
        for name in (("ingest", "k_pre") if r % 2 == 0 else ("k_pre", "ingest")):
            ms, launches[name] = k_pre_ms(det, legs[name])
            pre[name].append(ms)
    # feed (b)'s own ingest (frame-sized BGR + u16 depth, a plain copy) and what the call costs the host thread
    copy_ms = [k_pre_ms(det, lambda: det.upload_device(dev_prepared[0]))[0] for _ in range(3)]
    call_s = 0.0
    for i in range(60):          # the device idle before every call: the host side alone, no wait for an earlier ingest
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det.upload_device(dev_prepared[i % len(dev_prepared)])
        call_s += time.perf_counter() - t0
    call_us = call_s / 60 * 1e6
    det.close()
    torch.cuda.synchronize()

    print("device_input_rate  %s  %s  device %s" % (time.strftime("%Y-%m-%d %H:%M"), platform.node(), torch.cuda.get_device_name(0)))
    print("default workload: %dx%d RGB-D, %d templates, threshold %g, %d frames per step, three device lanes; %d steps per run, median of %d alternating rounds"
          % (W, H, N_TEMPLATES, THR, B, args.steps, args.rounds))
    print("%-44s %12s %12s   %s" % ("feed", "steps/s", "frames/s", "steps/s over the rounds"))
    names = {"resident": "(a) resident, no upload", "device": "(b) upload_device, fresh device tensors", "pageable": "(c) upload, fresh pageable host frames"}
    for feed in ("resident", "device", "pageable"):
        print("%-44s %12.1f %12.0f   %s   (%.1f matches per frame)" % (names[feed], med(feeds[feed]), med(feeds[feed]) * B, spread(feeds[feed]), matches[feed]))
    a, b, c = (med(feeds[k]) for k in ("resident", "device", "pageable"))
    print("ratios: (b) / (c) = %.2f, (b) / (a) = %.3f; one step costs %.3f ms resident and %.3f ms fed from device memory (+%.3f ms)"
          % (b / c, b / a, 1e3 / a, 1e3 / b, 1e3 / b - 1e3 / a))
    print("k_pre stage per step on %d raw %dx%d MONO8 + float-depth frames -> %dx%d (blur3, crop x = %d), device time:" % (B, RAW_W, H, W, H, CROP_X))
    for name, what in (("ingest", "upload_device: k_ingest"), ("k_pre", "upload_raw: k_pre_color + k_pre_depth")):
        print("  %-40s %8.4f ms   (%d launches per step; rounds %s)" % (what, med(pre[name]), launches[name], spread(pre[name])))
    print("  k_ingest / k_pre_* = %.3f" % (med(pre["ingest"]) / med(pre["k_pre"])))
    print("feed (b)'s ingest (frame-sized BGR + u16 depth, plain copy): %.4f ms device time per step (rounds %s); one upload_device call of %d frames"
          " keeps the host thread %.1f us (mean of 60 calls, the device idle before each)" % (med(copy_ms), spread(copy_ms), B, call_us))
    print("all rounds: " + json.dumps({"steps_per_s": feeds, "k_pre_ms_per_step": pre}))


if __name__ == "__main__":
    main()
