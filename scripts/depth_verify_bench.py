#!/usr/bin/env python3
"""The depth check of matches against device-resident template depth (DepthTemplates = lmx_depth_templates_* + lmx_depth_diff_matches) on the
2652-view memoryChip2 bank at 640x480:
  build      DepthTemplates.from_mesh over all 2652 views (render + crop on the device), cold and warm; device_bytes
  one frame  lmx_depth_diff_matches with 100, 1000 and 5000 matches (host clock around the call, which ends in a stream synchronise)
  64 frames  x 1000 matches in one call
  upload     the same calls with ONE match per frame: what a call costs before the kernel has work (scene staging + transfer, launch,
             read-back); its share of the full call
  host       the same header (csrc/lmx_depth_verify.hpp) built with g++ -O3, one core, the same inputs; the results must be equal
  bytes      what the kernel has to move per call, from the shapes: padded crop bytes + 2 bytes per crop pixel on the object that lies
             inside the scene + 32 bytes per match; over the kernel's time this is its achieved rate (kernel time: a separate run under
             `rocprofv3 --kernel-trace --stats -- python scripts/depth_verify_bench.py --kernels`; the difference of the two host clocks
             printed here is an estimate only)
Matches are placed at random positions with the crop fully inside the frame, random templates (seeded).  Needs a GPU.
usage: depth_verify_bench.py [--repeats 30] [--kernels]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
HBM_MEASURED = 6.29e12   # bytes/s, float4 copy (MI355X_MICROARCH.md); spec 8.0e12


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


class HostDiff:
    """csrc/lmx_depth_verify.hpp built for the host (tests/cpp/depth_verify_host.cpp, g++ -O3) over a list of uint16 [h, w] crops: one
    core.  Calling it gives int64 [n, 3] rows (sum_abs_mm, n_valid, n_template) for the matches of contiguous frames of one size."""

    def __init__(self, crops):
        with tempfile.TemporaryDirectory() as tmp:
            so = os.path.join(tmp, "libdvhost.so")
            subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc"),
                                   "-o", so, os.path.join(ROOT, "tests", "cpp", "depth_verify_host.cpp")])
            self.lib = C.CDLL(so)
        vp = C.c_void_p
        self.lib.dv_host_pitch.argtypes = [C.c_int]
        self.lib.dv_host_pitch.restype = C.c_int
        self.lib.dv_host_diff_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]
        self.lib.dv_host_diff_batch.restype = None
        self.pads = []                                                  # rows zero-padded to the pitch the device atlas uses
        for c in crops:
            c = np.asarray(c, np.uint16)
            assert c.ndim == 2
            p = np.zeros((c.shape[0], self.lib.dv_host_pitch(c.shape[1])), np.uint16)
            p[:, :c.shape[1]] = c
            self.pads.append(p)
        self.ptrs = (C.c_void_p * max(1, len(self.pads)))(*[p.ctypes.data for p in self.pads])
        self.ws = np.asarray([np.shape(c)[1] for c in crops], np.int32)
        self.hs = np.asarray([p.shape[0] for p in self.pads], np.int32)
        self.ps = np.asarray([p.shape[1] for p in self.pads], np.int32)

    def __call__(self, frames, m, offs, vectors):
        out = np.zeros((len(m), 3), np.int64)
        for f, frame in enumerate(frames):
            a, b = int(offs[f]), int(offs[f + 1])
            if a == b:
                continue
            assert frame.dtype == np.uint16 and frame.flags.c_contiguous
            jobs = np.ascontiguousarray(np.stack([m["x"][a:b], m["y"][a:b], m["template_id"][a:b]], 1), np.int32)
            res = out[a:b]                                              # a contiguous view: rows a..b of a C-ordered array
            self.lib.dv_host_diff_batch(self.ptrs, self.ws.ctypes.data, self.hs.ctypes.data, self.ps.ctypes.data, frame.ctypes.data, frame.shape[1],
                                        frame.shape[0], jobs.ctypes.data, b - a, int(vectors), res.ctypes.data)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--kernels", action="store_true", help="only the device calls, a fixed number of times each: the program for rocprofv3")
    args = ap.parse_args()
    from linemod_pose_estimation_amd import MATCH_DTYPE, DepthTemplates, meshsynth as ms
    F = ms.ENSENSO["fx"]
    chip, views = ms.load_mesh("memoryChip2"), ms.view_grid()
    assert len(views) == 2652
    t0 = time.perf_counter()
    t = DepthTemplates.from_mesh(chip, views, W, H, F, F)
    cold = time.perf_counter() - t0
    t.close()
    t0 = time.perf_counter()
    t = DepthTemplates.from_mesh(chip, views, W, H, F, F)
    warm = time.perf_counter() - t0
    rects = np.asarray([t.rect(i) for i in range(len(t))], np.int64)
    padded = int((rects[:, 3] * ((rects[:, 2] + 7) // 8 * 8) * 2).sum())
    print("from_mesh, 2652 views of memoryChip2 at %dx%d: %.3f s first call (creates the stream, loads the code objects), %.3f s second call = %.0f views/s"
          % (W, H, cold, warm, 2652 / warm))
    print("device_bytes %d = %.1f MB (padded crops %d + 24 per template); whole frames would be %.0f MB; mean crop %.0f x %.0f"
          % (t.device_bytes, t.device_bytes / 1e6, padded, 2652 * W * H * 2 / 1e6, rects[:, 2].mean(), rects[:, 3].mean()))

    rng = np.random.default_rng(5)
    base = ms.make_scene(chip, views, W, H, seed=3, n_instances=3)[0][1]
    frames = [np.ascontiguousarray(np.roll(base, 7 * f, axis=1)) for f in range(64)]

    def draw(n):
        m = np.zeros(n, MATCH_DTYPE)
        tid = rng.integers(0, len(t), n)
        m["template_id"] = tid
        m["x"] = (rng.random(n) * (W - rects[tid, 2] + 1)).astype(np.int64)
        m["y"] = (rng.random(n) * (H - rects[tid, 3] + 1)).astype(np.int64)
        m["similarity"] = 90.0
        return m

    def kernel_bytes(m, d):
        tid = m["template_id"]
        return int((rects[tid, 3] * ((rects[tid, 2] + 7) // 8 * 8) * 2).sum() + 2 * d["n_template"].astype(np.int64).sum() + 32 * len(m))

    cases = [("1 frame x %d matches" % n, frames[:1], draw(n), [0, n]) for n in (100, 1000, 5000)]
    cases.append(("64 frames x 1000 matches", frames, draw(64000), [1000 * f for f in range(65)]))
    if args.kernels:
        for name, fr, m, offs in cases:
            for _ in range(10):
                t.diff(fr, m, offs)
        print("--kernels: every case 10 times")
        return

    host = HostDiff([t.crop(i) for i in range(len(t))])

    for name, fr, m, offs in cases:
        d = t.diff(fr, m, offs)
        ref = host(fr, m, offs, 1)
        assert np.array_equal(np.stack([d["sum_abs_mm"], d["n_valid"], d["n_template"]], 1), ref), name
        full = timed(lambda: t.diff(fr, m, offs), args.repeats)
        one = m[np.asarray(offs[:-1])]                                  # one match per frame: the call without kernel work to speak of
        one_offs = list(range(len(fr) + 1))
        floor = timed(lambda: t.diff(fr, one, one_offs), args.repeats)
        reps = max(2, args.repeats // 10)
        hv = timed(lambda: host(fr, m, offs, 1), reps, warmup=1)
        hp = timed(lambda: host(fr, m, offs, 0), reps, warmup=1)
        nbytes = kernel_bytes(m, d)
        est = max(full[0] - floor[0], 1e-9)
        print("%s: call %.3f ms median (min %.3f, max %.3f) = %.2f us per match" % (name, 1e3 * full[0], 1e3 * full[1], 1e3 * full[2], 1e6 * full[0] / len(m)))
        print("    one match per frame (scene staging + upload of %.1f MB, launch, read-back): %.3f ms median = %.0f %% of the full call"
              % (len(fr) * W * H * 2 / 1e6, 1e3 * floor[0], 100 * floor[0] / full[0]))
        print("    kernel bytes from the shapes: %.1f MB; over the difference of the two medians (%.3f ms, an estimate, not a kernel trace): %.2f TB/s"
              " = %.0f %% of the measured HBM copy rate (6.29 TB/s; the crops of a call are read once each and may come from the L2 / Infinity Cache)"
              % (nbytes / 1e6, 1e3 * est, nbytes / est / 1e12, 100 * nbytes / est / HBM_MEASURED))
        print("    host, one core, same header: %.1f ms walking vectors, %.1f ms pixel by pixel -> device call %.0f x / %.0f x faster; results equal"
              % (1e3 * hv[0], 1e3 * hp[0], hv[0] / full[0], hp[0] / full[0]))
    t.close()


if __name__ == "__main__":
    main()
