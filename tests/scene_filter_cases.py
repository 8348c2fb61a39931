"""The scene's depth outlier filter (csrc/lmx_scene_filter.hpp) restated in numpy by brute force -- every window's distances are sorted and
the first k summed, where the header bisects -- and the frames the CPU and GPU tests share: small frames where the definition can go
wrong, and three constructed scenes with planted outliers."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

import pose_refine_cases as prc

HOST_SRC = os.path.join(prc.ROOT, "tests", "cpp", "scene_filter_host.cpp")
MAIN_SRC = os.path.join(prc.ROOT, "tests", "cpp", "scene_filter_main.cpp")
HOST_FLAGS = prc.HOST_FLAGS

MAX_Q = (1 << 20) - 1
MAX_DIFF = 1 << 14
FAR_MM = 2.0 ** 21
INFO_FIELDS = ("n_valid", "n_sparse", "n_scored", "n_removed", "sum_q", "sum_qq", "threshold")
INFO_DTYPE = np.dtype([(k, "<i8") for k in INFO_FIELDS[:-1]] + [("threshold", "<f8")])
CAM = (570.0, 570.0)   # fx, fy of the constructed scenes; cx = W / 2, cy = H / 2
INVALID, SPARSE, SCORED = 0, 1, 2


def np_points(scene, cam):
    """-> (P int64 [H, W, 3], has_point bool [H, W])."""
    H, W = scene.shape
    fx, fy, cx, cy = [np.float64(v) for v in cam]
    ifx, ify = np.float64(1.0) / fx, np.float64(1.0) / fy
    Y, X = np.mgrid[0:H, 0:W]
    z = scene.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        qx = ((X.astype(np.float64) - cx) * z) * ifx
        qy = ((Y.astype(np.float64) - cy) * z) * ify
        has = (scene != 0) & (np.abs(qx) <= FAR_MM) & (np.abs(qy) <= FAR_MM)
    P = np.zeros((H, W, 3), np.int64)
    P[..., 0][has] = np.rint(16.0 * qx[has]).astype(np.int64)
    P[..., 1][has] = np.rint(16.0 * qy[has]).astype(np.int64)
    P[..., 2][has] = 16 * scene[has].astype(np.int64)
    return P, has


def np_isqrt(a):
    d = np.floor(np.sqrt(a.astype(np.float64))).astype(np.int64)
    d = np.where(d * d > a, d - 1, d)
    return np.where((d + 1) * (d + 1) <= a, d + 1, d)


def np_filter(scene, cam, r=3, k=15, mul=1.0):
    """-> (filtered uint16 [H, W], record dict, q int64 [H, W], state int8 [H, W])."""
    scene = np.ascontiguousarray(scene, np.uint16)
    H, W = scene.shape
    P, has = np_points(scene, cam)
    big = np.int64(1) << 40
    Pp = np.zeros((H + 2 * r, W + 2 * r, 3), np.int64)
    hp = np.zeros((H + 2 * r, W + 2 * r), bool)
    Pp[r:r + H, r:r + W] = P
    hp[r:r + H, r:r + W] = has
    dist = []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            D = Pp[r + dy:r + dy + H, r + dx:r + dx + W] - P
            ok = has & hp[r + dy:r + dy + H, r + dx:r + dx + W] & (np.abs(D) <= MAX_DIFF).all(-1)
            dist.append(np.where(ok, np_isqrt((D * D).sum(-1)), big))
    dist = np.sort(np.stack(dist), axis=0)
    n_nb = (dist < big).sum(0)
    S = dist[:k].sum(0)
    valid = scene != 0
    scored = valid & (n_nb >= k)
    state = np.where(scored, SCORED, np.where(valid, SPARSE, INVALID)).astype(np.int8)
    q = np.zeros((H, W), np.int64)
    q[scored] = np.minimum((S[scored] << 16) // (k * scene[scored].astype(np.int64)), MAX_Q)
    n, sq, sqq = int(scored.sum()), int(q[scored].sum()), int((q[scored] * q[scored]).sum())
    if n < 2:
        thr = 2.0 ** 20
    else:
        N, fsq = float(n), float(sq)
        mean = fsq / N
        var = (float(sqq) - (fsq * fsq) / N) / (N - 1.0)
        thr = mean + float(mul) * math.sqrt(var if var > 0.0 else 0.0)
    kept = scored & (q.astype(np.float64) <= thr)
    rec = dict(n_valid=int(valid.sum()), n_sparse=int((state == SPARSE).sum()), n_scored=n, n_removed=int((scored & ~kept).sum()), sum_q=sq, sum_qq=sqq,
               threshold=float(thr))
    return np.where(kept, scene, 0).astype(np.uint16), rec, q, state


def record_array(rec):
    a = np.zeros(1, INFO_DTYPE)
    for k in INFO_FIELDS:
        a[k] = rec[k]
    return a


# ---- the header on the CPU -------------------------------------------------------------------------------------------------------------------

def build_host(directory, opt=None):
    so = os.path.join(str(directory), "libsfhost.so")
    subprocess.check_call(["g++"] + HOST_FLAGS + ([opt] if opt else []) + ["-fPIC", "-shared", "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.sf_host_filter.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, vp, vp]
    return lib


def host_filter(lib, scene, cam, r=3, k=15, mul=1.0):
    """-> (rc, filtered, record array [1]); rc 1: the parameters are refused, 2: the frame is too large."""
    scene = np.ascontiguousarray(scene, np.uint16)
    H, W = scene.shape
    v = np.asarray(list(cam) + [mul], np.float64)
    out = np.full((H, W), 0x7777, np.uint16)
    info = np.zeros(1, INFO_DTYPE)
    rc = lib.sf_host_filter(scene.ctypes.data, W, H, W, v.ctypes.data, int(r), int(k), out.ctypes.data, info.ctypes.data)
    return rc, out, info


# ---- frames ------------------------------------------------------------------------------------------------------------------------------------

def noisy(W, H, seed, holes=0.05, spikes=6):
    """A slanted surface with a little noise, holes and a few pixels well in front of it."""
    rng = np.random.default_rng(seed)
    Y, X = np.mgrid[0:H, 0:W]
    s = (700 + 2 * X + Y + rng.integers(0, 4, (H, W))).astype(np.uint16)
    s[rng.random((H, W)) < holes] = 0
    for _ in range(spikes):
        s[rng.integers(0, H), rng.integers(0, W)] = 620
    return s


def lattice(W, H):
    """z = 1024 under fx = fy = 512: the points lie 32 ticks apart exactly, so the distances are 32, 45 (diagonal), 64, .."""
    return np.full((H, W), 1024, np.uint16), (512.0, 512.0, 4.0, 4.0)


@functools.lru_cache(maxsize=None)
def small_cases():
    """-> [(name, scene, camera, r, k, stddev_mul)]"""
    def cam(s):
        return CAM + (s.shape[1] / 2.0, s.shape[0] / 2.0)

    out = []

    def add(name, s, r=3, k=15, mul=1.0, c=None):
        s = np.ascontiguousarray(s, np.uint16)
        out.append((name, s, c if c is not None else cam(s), r, k, mul))

    add("1x1", np.full((1, 1), 500))
    add("3x3_r1_k3", np.full((3, 3), 500), r=1, k=3)
    add("5x4_r3", 600 + np.arange(20).reshape(4, 5))                        # narrower than the window
    add("41x37", noisy(41, 37, 1))
    add("33x9", noisy(33, 9, 2))
    add("all_zero", np.zeros((6, 7)))
    add("one_scored", np.full((3, 3), 500), r=1, k=8)                        # only the centre has 8 neighbours: n < 2
    lat, lcam = lattice(6, 5)
    add("all_q_equal", lat, r=1, k=1, c=lcam)                                # every nearest neighbour is 32 ticks away: var = 0
    add("r7_k224", noisy(17, 16, 3, holes=0.0, spikes=1), r=7, k=224)       # 3 x 2 pixels have a whole window
    add("r7_k1", noisy(17, 16, 3, holes=0.0, spikes=1), r=7, k=1)
    add("ties_k2", lat, r=1, k=2, c=lcam)                                    # the 2 smallest of four distances of 32
    add("ties_k6", lat, r=1, k=6, c=lcam)                                    # four of 32, then 2 of the four of 45
    at = np.full((3, 3), 2024)
    at[1, 1] = 1000
    add("bound_at", at, r=1, k=8)                                            # |D.z| = 2^14 exactly: a neighbour
    beyond = at.copy()
    beyond[0, 2] = 2025
    add("bound_beyond", beyond, r=1, k=8)                                    # |D.z| = 2^14 + 16: none, by that bound alone
    add("clamp", np.asarray([[900, 900, 900], [900, 1, 65535], [900, 900, 65535]]), r=1, k=2)
    add("far", np.full((5, 6), 800), r=1, k=1, c=(1e-4, 1e-4, 3.0, 2.0))     # only the pixel at column 3, row 2 has a point
    add("mul_0", noisy(41, 37, 1), mul=0.0)
    add("mul_16", noisy(41, 37, 1), mul=16.0)
    return out


def constructed_scenes():
    """Three scenes with planted outliers -> [(name, scene, planted [(row, col)])], for the camera CAM + (W / 2, H / 2) and the default
    parameters: a flat wall at 800 mm and one slanted by 3 mm a column, each 40 x 32 with a 3 x 3 hole and five pixels 60 mm in front of the
    surface; a box at 700 mm in front of a wall at 1000 mm, 48 x 40, with three pixels at 850 mm on the box's outline."""
    planted = [(10, 10), (10, 11), (20, 30), (5, 25), (16, 3)]
    out = []
    for name, slope in (("flat", 0), ("slanted", 3)):
        Y, X = np.mgrid[0:32, 0:40]
        s = (800 + slope * X).astype(np.uint16)
        for p in planted:
            s[p] -= 60
        s[12:15, 20:23] = 0
        out.append((name, s, planted))
    s = np.full((40, 48), 1000, np.uint16)
    s[10:30, 12:36] = 700
    fly = [(10, 11), (20, 36), (30, 20)]
    for p in fly:
        s[p] = 850
    out.append(("box_on_wall", s, fly))
    return out


def scene_camera(s):
    return CAM + (s.shape[1] / 2.0, s.shape[0] / 2.0)


def two_frames():
    """Two frames of one size whose statistics differ: sums must not mix between frames."""
    far = noisy(45, 35, 6, holes=0.2, spikes=20)
    far[far != 0] += 300
    return [noisy(45, 35, 5), far]


def large_frame():
    return noisy(321, 241, 7, holes=0.02, spikes=60)
