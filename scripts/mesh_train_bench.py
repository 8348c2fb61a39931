#!/usr/bin/env python3
"""Training a bank from a mesh: the batched device path (NativeBank.train_mesh = lmx_bank_train_mesh: rasteriser + quantisers + packed
read-back on the device, host selection on a few threads) against the per-view path it replaces (meshsynth.train_bank: CPU render of every
view, NativeBank.add_template per view).  One box, one process, same run:
  baseline   meshsynth.train_bank(NativeBank.add_template) over the first 442 views of memoryChip2, 640x480 RGB-D, warm
  feature    train_mesh on the same 442 views, and on all 2652; the banks must be equal
  required   feature >= 5 x baseline in views/s (the per-view path spends ~5/6 of its time rendering on the host: below 5 x the new path
             would still cost more per view than add_template alone)
and, from lmx_bank_train_mesh's own clock (LMX_MESH_TRAIN_TIMING=1), where a call's wall time goes: waiting for the device, host selection.
--kernels: only run train_mesh on all 2652 views twice (the program for `rocprofv3 --kernel-trace --stats -- python scripts/mesh_train_bench.py
--kernels`: kernel time per view = the k_mesh_* / k_color_quantize / k_depth_quantize totals divided by 2 x 2652).
--device-candidates: the same with the candidates found and compacted on the device (device_candidates=True).
Needs a GPU.  usage: mesh_train_bench.py [--rounds 3] [--kernels] [--device-candidates]"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fresh():
    from linemod_pose_estimation_amd import NativeBank, meshsynth as ms
    b = ms.empty_bank()
    return NativeBank.create(b.T, b.modalities)


def same(a, b):
    a, b = a.to_bank(), b.to_bank()
    return all(np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a.classes, b.classes)) and len(a.classes) == len(b.classes)


def timed_train_mesh(tri, views, device_candidates=False):
    """-> (seconds, bank, the library's timing line as a dict)."""
    nb = fresh()
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            nb.train_mesh(tri, views, device_candidates=device_candidates)
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    line = [ln for ln in text.splitlines() if "lmx_bank_train_mesh timing" in ln]
    info = {k: float(v) for k, v in re.findall(r"(\w+) ([0-9.]+)", line[-1])} if line else {}
    return dt, nb, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--device-candidates", action="store_true", help="train_mesh with device_candidates=True (lmx_bank_train_mesh_opts, LMX_TRAIN_CANDIDATES_DEVICE)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_train_bench.py needs a GPU")
    os.environ["LMX_MESH_TRAIN_TIMING"] = "1"
    from linemod_pose_estimation_amd import meshsynth as ms
    chip, views = ms.load_mesh("memoryChip2"), ms.view_grid()
    first = views[:442]
    if args.kernels:
        for _ in range(2):
            dt, _, info = timed_train_mesh(chip, views, args.device_candidates)
            print("train_mesh 2652 views: %.3f s  %s" % (dt, info))
        return
    # warm: device, library, the C rasteriser
    ms.train_bank(fresh().add_template, chip, first[:8])
    timed_train_mesh(chip, first[:40], args.device_candidates)
    base, feat, full, infos = [], [], [], []
    ref = None
    for r in range(args.rounds):
        nb = fresh()
        t0 = time.perf_counter()
        meta = ms.train_bank(nb.add_template, chip, first)
        base.append(len(first) / (time.perf_counter() - t0))
        ref = nb
        dt, got, _ = timed_train_mesh(chip, first, args.device_candidates)
        feat.append(len(first) / dt)
        assert len(meta) == 442 and same(got, ref), "train_mesh differs from the per-view loop"
        dt, _, info = timed_train_mesh(chip, views, args.device_candidates)
        full.append(len(views) / dt)
        infos.append(info)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    ratio = med(feat) / med(base)
    print("mesh_train_bench  %s  device %s" % (time.strftime("%Y-%m-%d %H:%M"), torch.cuda.get_device_name(0)))
    print("memoryChip2 (%d triangles), 640x480, ColorGradient + DepthNormal, T = (5, 8); median of %d rounds; candidates on the %s" %
          (len(chip), args.rounds, "device" if args.device_candidates else "host"))
    print("%-58s %12.1f views/s  (%.3f ms per view)" % ("baseline: meshsynth.train_bank(add_template), 442 views", med(base), 1e3 / med(base)))
    print("%-58s %12.1f views/s  (%.3f ms per view)" % ("feature:  train_mesh, the same 442 views", med(feat), 1e3 / med(feat)))
    print("%-58s %12.1f views/s  (%.3f ms per view)" % ("feature:  train_mesh, all 2652 views", med(full), 1e3 / med(full)))
    print("feature / baseline on 442 views: %.1f x   (required: >= 5 x)   banks equal: yes" % ratio)
    i = infos[-1]
    if i:
        print("inside the 2652-view call: total %.1f ms, waiting for the device %.1f ms, host selection %.1f ms on %d threads (%.0f %% of the call), "
              "%d batches of %d views" % (i["total_ms"], i["device_wait_ms"], i["host_select_ms"], int(i["threads"]) if "threads" in i else 8,
                                          100.0 * i["host_select_ms"] / i["total_ms"], int(i["batches"]), int(i.get("of", 32))))
        print("device memory of the call: %.1f MB, pinned read-back buffers: %.1f MB" % (i["device_bytes"] / 1e6, i["pinned_bytes"] / 1e6))
        if args.device_candidates:
            print("candidate lists: %d device views, %d fallback views, %d candidates, %.1f MB read back" %
                  (int(i["device_views"]), int(i["fallback_views"]), int(i["n_candidates"]), i["list_bytes"] / 1e6))
    print("all rounds: baseline %s  feature442 %s  feature2652 %s" % ([round(x, 1) for x in base], [round(x, 1) for x in feat], [round(x, 1) for x in full]))
    assert ratio >= 5.0, "train_mesh is only %.2f x the per-view path" % ratio


if __name__ == "__main__":
    main()
