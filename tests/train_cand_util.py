"""Shared by tests/test_train_cand_host.py and tests/test_gpu_train_candidates.py: the windows of train_select_cases (every level and modality
of every case as one whole-image window), the candidate list of a window restated in numpy from the definitions in csrc/lmx_train_cand.hpp
(np_restatement's brute-force chessboard distance and erode3, not the AND steps), and the CPU build of that header behind ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import np_restatement as R
import train_select_cases as tc
from conftest import ROOT

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
NO_ZERO = float(1 << 28)
HEADER_WORDS = 16


def build_shim(directory):
    so = os.path.join(str(directory), "libtchost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "cpp", "train_cand_host.cpp")])
    lib = C.CDLL(so)
    lib.tch_window.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.tch_select.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def windows(cases):
    """-> list of dicts, one per (case, level, modality): color, label, mag, mask, nf, strong, et (the level's), case index, family, name."""
    out = []
    for ci, c in enumerate(cases):
        for l in range(len(c["labels"])):
            for m, mod in enumerate(c["mods"]):
                color = mod["type"] == "ColorGradient"
                out.append({"case": ci, "family": c["family"], "name": "%s/L%d/M%d" % (c["name"], l, m), "color": color,
                            "label": np.ascontiguousarray(c["labels"][l][m], np.uint8),
                            "mag": np.ascontiguousarray(c["mags"][l][m], np.float32) if color else None,
                            "mask": None if c["masks"] is None else np.ascontiguousarray(c["masks"][l], np.uint8),
                            "nf": mod["num_features"] >> l, "strong": float(mod.get("strong_threshold", tc.STRONG)),
                            "et": int(mod.get("extract_threshold", 2)) >> l})
    return out


def window(color, label, mag=None, mask=None, nf=4, strong=tc.STRONG, et=2, name="window"):
    return {"case": -1, "family": "shapes", "name": name, "color": color, "label": np.ascontiguousarray(label, np.uint8),
            "mag": None if mag is None else np.ascontiguousarray(mag, np.float32), "mask": None if mask is None else np.ascontiguousarray(mask, np.uint8),
            "nf": nf, "strong": float(strong), "et": int(et)}


def special_windows():
    """Windows at which the packed AND steps and the in-order compaction in particular can go wrong (see the tests that use them)."""
    rng = np.random.default_rng(31)
    out = []
    for h in (1, 2, 7):
        for w in (1, 2, 3, 5, 63, 65):
            mask = None if (h + w) % 2 else (rng.random((h, w)) < 0.9).astype(np.uint8) * 255
            for et in (0, 1, 2):
                out.append(window(False, tc.blocks(rng, h, w, 3), None, mask, 1, et=et, name="depth_%dx%d_et%d" % (w, h, et)))
            out.append(window(True, tc.angles(rng, h, w, 0.9), tc.magnitudes(rng, h, w, 0.8), mask, 1, name="color_%dx%d" % (w, h)))
    uniform = np.full((8, 8), 16, np.uint8)
    out.append(window(False, uniform, None, None, 4, et=2, name="uniform_8x8"))
    sprinkled = uniform.copy()
    sprinkled[rng.random((8, 8)) < 0.15] = 255
    sprinkled[2, 5] = sprinkled[6, 1] = 0
    sprinkled[0, 0] = 2          # a second label: its plane is zero wherever there is no 255
    out.append(window(False, sprinkled, None, None, 4, et=1, name="sprinkled_8x8"))
    only255 = uniform.copy()
    only255[rng.random((8, 8)) < 0.2] = 255
    out.append(window(False, only255, None, None, 4, et=2, name="uniform_255_8x8"))
    strip = np.full((3, 520), 8, np.uint8)
    strip[1, 0] = 0
    out.append(window(False, strip, None, None, 8, et=2, name="strip_520x3"))
    for value in (1, 128):
        mask = np.zeros((20, 27), np.uint8)
        mask[3:17, 4:22] = value
        mask[8:11, 9:12] = 0     # a hole: inner contour, distances from the inside
        out.append(window(False, tc.blocks(rng, 20, 27, 5), None, mask, 4, et=1, name="depth_mask_%d" % value))
        out.append(window(True, tc.angles(rng, 20, 27, 0.95), tc.magnitudes(rng, 20, 27, 0.9), mask, 4, name="color_mask_%d" % value))
    grades = np.zeros((20, 27), np.uint8)
    grades[2:18, 3:24] = rng.integers(1, 256, (16, 21))
    out.append(window(True, tc.angles(rng, 20, 27, 0.95), tc.magnitudes(rng, 20, 27, 0.9), grades, 4, name="color_mask_random_values"))
    corner = np.full((256, 256), 32, np.uint8)      # the largest square window the device path takes; distances up to 255
    corner[255, 255] = 0
    out.append(window(False, corner, None, None, 8, et=2, name="corner_256x256"))
    return out


def restate(w):
    """The list of one window from the definitions -> (xs, ys, labels, scores float32, label_counts int [8], area)."""
    label = w["label"]
    if w["color"]:
        ok = (label > 0) & (w["mag"] > np.float32(w["strong"]) * np.float32(w["strong"]))
        if w["mask"] is not None:
            m = w["mask"]
            ok &= m.astype(np.int32) > R.erode3(m).astype(np.int32)
        ys, xs = np.nonzero(ok)
        labels = np.asarray([int(v).bit_length() - 1 if v & (v - 1) == 0 else -1 for v in label[ys, xs].astype(int)], np.int64)
        return xs, ys, labels, w["mag"][ys, xs], np.zeros(8, np.int64), 0
    inside = np.ones(label.shape, bool) if w["mask"] is None else R.erode3(R.erode3(w["mask"])) > 0
    score = np.zeros(label.shape, np.float32)
    lab = np.full(label.shape, -1)
    for k in range(8):
        here = inside & (label == (1 << k))
        if here.any():
            d = R.chessboard_distance(np.where(inside, label & (1 << k), 0))
            score[here], lab[here] = d[here], k
    ok = (lab >= 0) & (score >= np.float32(w["et"]))
    ys, xs = np.nonzero(ok)
    return xs, ys, lab[ys, xs], score[ys, xs], np.bincount(lab[ys, xs], minlength=8), int(inside.sum())


def decode(records, n):
    """records uint32 [cap, 2] -> (xs, ys, labels, scores) of the first n"""
    r = records[:n]
    lab = (r[:, 0] >> 28).astype(np.int64)
    return (r[:, 0] & 0x3fff).astype(np.int64), (r[:, 0] >> 14 & 0x3fff).astype(np.int64), np.where(lab > 7, -1, lab), r[:, 1].copy().view(np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data


def cpu_list(lib, w):
    """tch_window -> (n, records, header)"""
    h, wd = w["label"].shape
    records = np.zeros((h * wd + 1, 2), np.uint32)
    header = np.zeros(HEADER_WORDS, np.uint32)
    n = lib.tch_window(int(w["color"]), _ptr(w["label"]), _ptr(w["mag"]), _ptr(w["mask"]), h, wd, w["strong"], w["et"], _ptr(records), h * wd, _ptr(header))
    return n, records, header


def cpu_select(lib, w, records, header):
    """tch_select -> None (rejected) or features int32 [nf, 3]"""
    feats = np.zeros((64, 3), np.int32)
    n = lib.tch_select(int(w["color"]), _ptr(records), _ptr(header), w["nf"], _ptr(feats))
    assert n == -1 or n == w["nf"], (w["name"], n)
    return None if n < 0 else feats[:n].copy()


def same_list(got, ref, what):
    """got: (n, records, header); ref: restate()'s tuple"""
    n, records, header = got
    xs, ys, labels, scores, counts, area = ref
    assert n == len(xs) == header[0], (what, n, len(xs), header[0])
    gx, gy, gl, gs = decode(records, n)
    assert np.array_equal(gx, xs) and np.array_equal(gy, ys), (what, "positions / raster order")
    assert np.array_equal(gl, labels), (what, "labels")
    assert np.array_equal(gs, scores.astype(np.float32)), (what, "scores", gs[:8], scores[:8])
    assert header[1] == area and np.array_equal(header[2:10].astype(np.int64), counts), (what, header[:10], area, counts)
    assert header[10] == 0
