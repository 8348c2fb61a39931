#!/usr/bin/env python3
"""Gray (LMX_CTX_GRAY, one colour plane) against BGR (the gray frame copied into three channels) on BASELINE configs[0]: 640x480,
ColorGradient only, 3000 templates, threshold 92, batches of 64 frames on device lanes.  One process, one box, the two kinds in
alternating runs (--rounds of each), every line the median of its rounds:
  resident   frames already on the device (the kernels alone)
  pageable   fresh pageable host frames every step (the host -> device boundary)
  raw_mono   raw MONO8 752x480 camera frames through lmx_ctx_upload_raw (3x3 blur + crop on the device); the BGR context replicates
             the plane into three channels there (the bench's config0_cg_only.raw_mono_752x480 line), the gray one keeps one
  one_frame  lmx_match with one fresh host frame per call (the reference's own pattern), microseconds per call
and the per-kernel time of k_color_quantize and k_pre (HIP events around every kernel, one batch in flight).  --tiles also times
k_color_quantize with each tile height pinned (LMX_COLOR_TILE=16 / 32, read when a context is created: one child process each).
Needs a GPU.  usage: gray_path_bench.py [--rounds 3] [--steps 30] [--tiles]"""
import argparse
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (timing helpers: run_pipelined, secondary_line)

W, H, B, THR, N_TEMPLATES = 640, 480, 64, 92.0, 3000


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def workload():
    from linemod_pose_estimation_amd import synth
    bank = synth.make_bank(N_TEMPLATES, modalities=("ColorGradient",), T=(5, 8), seed=20250214)
    scenes = [synth.make_scene(bank, W, H, seed=4000 + f, row_pad=0)[0] for f in range(B)]
    gray = [np.ascontiguousarray(s[0][:, :, 1]) for s in scenes]
    return bank, gray


def kernel_ms(det, n_frames, upload=None):
    det.set_profiling(True)
    det.reset_profiling()
    for _ in range(3):
        if upload:
            upload()
        det.enqueue(n_frames, THR)
        det.collect(n_frames)
    kt = {k: v[0] / 3.0 for k, v in det.kernel_times().items() if v[1]}
    det.set_profiling(False)
    return kt


def run_kind(torch, Detector, bank, gray, is_gray, steps):
    frames = [[g] if is_gray else [np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))] for g in gray]
    perms = [np.random.default_rng(s).permutation(B) for s in range(2)]
    host = [Detector.prepare_batch([[np.array(frames[i][0], copy=True)] for i in p]) for p in perms]
    mono = [np.ascontiguousarray(np.pad(g, ((0, 0), (56, 56)), mode="edge")) for g in gray]
    raw = [Detector.prepare_batch([[np.array(mono[i], copy=True)] for i in p]) for p in perms]
    out = {}
    line = bench.secondary_line(torch, Detector, bank, frames, B, THR, steps, breakdown=True, gray=is_gray)
    out["resident_fps"] = line["value"]
    out["k_color_quantize_ms_per_batch"] = line["kernel_ms_per_step"].get("k_color_quantize", 0.0)
    out["matches_per_frame"] = line["matches_per_frame"]
    out["pageable_fps"] = bench.secondary_line(torch, Detector, bank, None, B, THR, steps, uploads=host, gray=is_gray)["value"]

    def up_raw(det, i):
        det.upload_raw(raw[i % len(raw)], (752, 480), (56, 0), blur3=True, mono=True)
    out["raw_mono_fps"] = bench.secondary_line(torch, Detector, bank, None, B, THR, steps, uploads=up_raw, gray=is_gray)["value"]
    det = Detector(bank, W, H, max_batch=B, overlap=True, gray=is_gray)
    kt = kernel_ms(det, B, lambda: det.upload_raw(raw[0], (752, 480), (56, 0), blur3=True, mono=True))
    out["k_pre_ms_per_batch"] = kt.get("k_pre", 0.0)
    det.close()
    # one frame per call, a fresh host frame each time
    det = Detector(bank, W, H, max_batch=1, gray=is_gray)
    singles = [[np.array(frames[i][0], copy=True)] for i in range(16)]
    for i in range(20):
        det.match(singles[i % 16], THR)
    n = 300
    t0 = time.perf_counter()
    for i in range(n):
        det.match(singles[i % 16], THR)
    out["one_frame_us"] = (time.perf_counter() - t0) / n * 1e6
    det.close()
    return out


def tile_child(tile):
    """Child process: k_color_quantize per batch with LMX_COLOR_TILE pinned (set by the parent before this process started)."""
    import torch
    from linemod_pose_estimation_amd import Detector
    bank, gray = workload()
    res = {}
    for is_gray in (True, False, True, False):
        frames = [[g] if is_gray else [np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))] for g in gray]
        det = Detector(bank, W, H, max_batch=B, overlap=True, gray=is_gray)
        det.upload(frames)
        for _ in range(3):
            det.enqueue(B, THR)
            det.collect(B)
        res.setdefault("gray" if is_gray else "bgr", []).append(kernel_ms(det, B)["k_color_quantize"])
        det.close()
    torch.cuda.synchronize()
    print(json.dumps({"tile": tile, "k_color_quantize_ms_per_batch": {k: median(v) for k, v in res.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--tiles", action="store_true")
    ap.add_argument("--tile-child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tile_child:
        tile_child(args.tile_child)
        return
    import torch
    from linemod_pose_estimation_amd import Detector
    if not torch.cuda.is_available():
        raise SystemExit("gray_path_bench.py needs a GPU")
    bank, gray = workload()
    runs = {"gray": [], "bgr": []}
    for r in range(args.rounds):
        for kind in (("gray", "bgr") if r % 2 == 0 else ("bgr", "gray")):
            runs[kind].append(run_kind(torch, Detector, bank, gray, kind == "gray", args.steps))
    res = {k: {m: median([x[m] for x in v]) for m in v[0]} for k, v in runs.items()}
    print("gray_path_bench  %s  %s  device %s" % (time.strftime("%Y-%m-%d %H:%M"), platform.node(), torch.cuda.get_device_name(0)))
    print("BASELINE configs[0]: %dx%d, ColorGradient only, %d templates, threshold %g, %d frames per batch, device lanes; median of %d alternating rounds"
          % (W, H, N_TEMPLATES, THR, B, args.rounds))
    print("%-34s %14s %14s %10s" % ("", "gray (1 plane)", "BGR (3 planes)", "gray/BGR"))
    rows = [("resident frames/s", "resident_fps"), ("pageable host frames/s", "pageable_fps"), ("raw MONO8 752x480 frames/s", "raw_mono_fps"),
            ("one-frame call us", "one_frame_us"), ("k_color_quantize ms / 64 frames", "k_color_quantize_ms_per_batch"),
            ("k_pre ms / 64 raw frames", "k_pre_ms_per_batch"), ("matches per frame", "matches_per_frame")]
    for name, key in rows:
        g, b = res["gray"][key], res["bgr"][key]
        print("%-34s %14.3f %14.3f %10.3f" % (name, g, b, g / b if b else float("nan")))
    print("all rounds: " + json.dumps(runs))
    if args.tiles:
        for tile in (16, 32):
            env = dict(os.environ, LMX_COLOR_TILE=str(tile))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tile-child", str(tile)], env=env, capture_output=True, text=True,
                                 timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")]
            print("LMX_COLOR_TILE=%d: %s" % (tile, line[-1] if line else "failed (exit %d) %s" % (out.returncode, out.stderr[-300:])))
            if out.returncode != 0:
                break


if __name__ == "__main__":
    main()
