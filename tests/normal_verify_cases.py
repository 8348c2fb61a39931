"""The normal term of a match (lmx_normal_diff_matches): numpy restatements of csrc/lmx_normal_verify.hpp -- normal map, angle, match sums,
value -- in float32 operations in the written order, and the constructed depth images shared by tests/test_normal_verify_host.py (CPU build
of the header) and tests/test_gpu_normal_verify.py (the kernels).

Normal of a pixel: d = D[y][x]; invalid iff d == 0 or d >= distance_threshold; else DepthNormal's least squares over the eight taps at
offsets +-5 (reads outside give 0; a tap counts iff |tap - d| < difference_threshold), det / ddx / ddy in int64,
n = (fx * f32(ddx), fy * f32(ddy), -f32(det * d)), s = sqrt(nx*nx + ny*ny + nz*nz), invalid unless s > 0, q = rint((n * (1 / s)) * 16384)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import depth_verify_cases as dvc

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(_ROOT, "tests", "cpp", "normal_verify_host.cpp")
HOST_FLAGS = ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", os.path.join(_ROOT, "linemod_pose_estimation_amd", "csrc")]

F32 = np.float32
UNIT = 16384
DIFF_T, DIST_T = 50, 2000      # upstream's DepthNormal
FX = FY = 800.0


def np_angle_table():
    """llrint(2e6 * asin(min(1, i / 16384))) for i = 0 .. 16384, with numpy's arcsin."""
    i = np.arange(UNIT + 1, dtype=np.float64)
    return np.rint(2e6 * np.arcsin(np.minimum(1.0, i / float(UNIT)))).astype(np.uint32)


def np_normal_map(D, fx=FX, fy=FY, difference_threshold=DIFF_T, distance_threshold=DIST_T):
    """uint16 [H, W] -> int16 [H, W, 4] = (qx, qy, qz, valid), zeros where invalid."""
    H, W = D.shape
    P = np.zeros((H + 10, W + 10), np.int64)
    P[5:5 + H, 5:5 + W] = D
    d = P[5:5 + H, 5:5 + W]
    A0, A1, A3, b0, b1 = (np.zeros((H, W), np.int64) for _ in range(5))
    for oy in (-5, 0, 5):
        for ox in (-5, 0, 5):
            if ox == 0 and oy == 0:
                continue
            delta = P[5 + oy:5 + oy + H, 5 + ox:5 + ox + W] - d
            f = (np.abs(delta) < difference_threshold).astype(np.int64)
            A0 += f * ox * ox
            A1 += f * ox * oy
            A3 += f * oy * oy
            b0 += f * ox * delta
            b1 += f * oy * delta
    det = A0 * A3 - A1 * A1
    ddx = A3 * b0 - A1 * b1
    ddy = -A1 * b0 + A0 * b1
    nx = F32(fx) * ddx.astype(F32)
    ny = F32(fy) * ddy.astype(F32)
    nz = -((det * d).astype(F32))
    s = np.sqrt(nx * nx + ny * ny + nz * nz)
    ok = (d != 0) & (d < distance_threshold) & (s > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F32(1.0) / s
        q = [np.rint((n * inv) * F32(UNIT)) for n in (nx, ny, nz)]
    out = np.zeros((H, W, 4), np.int16)
    for c in range(3):
        out[..., c] = np.where(ok, q[c], 0).astype(np.int16)
    out[..., 3] = ok
    return out


def np_angle_index(a, b):
    """int16 [..., 4] stored normals (both valid) -> index into the angle table."""
    dlt = a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64)
    c2 = (dlt * dlt).sum(axis=-1)
    c = np.sqrt(c2.astype(F32))
    return np.minimum(UNIT, np.rint(c * F32(0.5)).astype(np.int64))


def np_normal_diff(crop, crop_n, scene, scene_n, x, y, table):
    """-> (sum_abs_mm, n_valid, n_template, sum_angle_urad, n_normal) as Python ints; x, y any Python ints."""
    h, w = crop.shape
    H, W = scene.shape
    x, y = int(x), int(y)
    n_template = int(np.count_nonzero(crop))
    j0, j1, i0, i1 = max(0, -x), min(w, W - x), max(0, -y), min(h, H - y)
    if j0 >= j1 or i0 >= i1:
        return 0, 0, n_template, 0, 0
    t = crop[i0:i1, j0:j1].astype(np.int64)
    s = scene[y + i0:y + i1, x + j0:x + j1].astype(np.int64)
    tn, sn = crop_n[i0:i1, j0:j1], scene_n[y + i0:y + i1, x + j0:x + j1]
    ok = (t != 0) & (s != 0)
    okn = ok & (tn[..., 3] != 0) & (sn[..., 3] != 0)
    ang = table[np_angle_index(tn, sn)].astype(np.int64)
    return int(np.abs(t - s)[ok].sum()), int(ok.sum()), n_template, int(ang[okn].sum()), int(okn.sum())


def np_value(sum_abs_mm, n_valid, sum_angle_urad, n_normal, no_value):
    if n_valid <= 0 or n_normal <= 0:
        return no_value
    return -(float(sum_abs_mm) / (float(n_valid) * 1000.0) + float(sum_angle_urad) / (float(n_normal) * 1e6))


def plane(w, h, c, a, b):
    """d = c + a x + b y as uint16 [h, w] (the caller keeps it inside 1 .. 65535)."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = c + a * xx + b * yy
    assert d.min() >= 1 and d.max() <= 65535
    return d.astype(np.uint16)


def plane_angle(fx, fy, a0, b0, d0, a1, b1, d1):
    """The angle in radians between the analytic normals (fx a, fy b, -d) of two plane pixels."""
    n0 = np.stack([fx * a0 * np.ones_like(d0, np.float64), fy * b0 * np.ones_like(d0, np.float64), -d0.astype(np.float64)], -1)
    n1 = np.stack([fx * a1 * np.ones_like(d1, np.float64), fy * b1 * np.ones_like(d1, np.float64), -d1.astype(np.float64)], -1)
    n0 /= np.linalg.norm(n0, axis=-1, keepdims=True)
    n1 /= np.linalg.norm(n1, axis=-1, keepdims=True)
    # through the chord: stable near 0 and near pi
    return 2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.linalg.norm(n0 - n1, axis=-1)))


OPPOSED = dict(w=64, h=64, c=100, a=9)     # d = 100 + 9 x against d = 100 + 9 (63 - x): about 178 degrees apart where d is near 100


def opposed_planes():
    o = OPPOSED
    up = plane(o["w"], o["h"], o["c"], o["a"], 0)
    return up, np.ascontiguousarray(up[:, ::-1])


@functools.lru_cache(maxsize=None)
def constructed_images():
    """-> list of (name, uint16 image).  Built once per session; treat as read-only."""
    rng = np.random.default_rng(20240611)
    out = []
    for a, b in ((0, 0), (1, 0), (0, 1), (3, -2), (-4, 5), (9, 0), (0, -9), (9, 9), (10, 0), (0, 10), (-10, 3), (11, -11)):
        # |slope| * 5 against difference_threshold 50: 9 keeps every tap (45 < 50), 10 is the first to drop them (50 is not < 50)
        out.append(("plane a=%d b=%d" % (a, b), plane(23, 19, 700, a, b)))
    out.append(("at distance_threshold - 1", np.full((13, 17), DIST_T - 1, np.uint16)))
    out.append(("at distance_threshold", np.full((13, 17), DIST_T, np.uint16)))
    out.append(("no measurement", np.zeros((13, 17), np.uint16)))
    step = np.full((21, 25), 900, np.uint16)
    step[:, 12:] = DIST_T - 1
    step[8:, :6] = DIST_T
    out.append(("steps across both thresholds", step))
    holes = plane(31, 27, 600, 2, 3)
    holes[rng.random(holes.shape) < 0.25] = 0
    out.append(("plane with holes", holes))
    noise = (800 + rng.integers(-60, 61, (29, 33))).astype(np.uint16)      # deltas on both sides of the difference threshold
    out.append(("noise around the difference threshold", noise))
    anyv = rng.integers(0, 65536, (16, 40)).astype(np.uint16)
    anyv[rng.random(anyv.shape) < 0.5] //= 64
    out.append(("any values", anyv))
    up, down = opposed_planes()
    out.append(("steep plane", up))
    out.append(("steep plane, opposed", down))
    for w in (11, 12, 64, 65, 70):
        for h in (11, 13, 37):
            out.append(("scene %dx%d" % (w, h), scene_image(w, h, rng)))
    return out


def scene_image(w, h, rng):
    """A surface with slopes on both sides of the tap limit, a far wall, holes."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = 900 + 4 * xx - 3 * yy + rng.integers(-12, 13, (h, w))
    d[:, w // 2:] += 7 * (xx[:, w // 2:] - w // 2)
    d[h // 3: h // 3 + 3, :] = DIST_T + 5
    d = d.astype(np.uint16)
    d[rng.random((h, w)) < 0.1] = 0
    return d


@functools.lru_cache(maxsize=None)
def wide():
    """The wide crops of depth_verify_cases.wide() against a 1200 x 12 scene_image -> (crops, crop normals, scene, scene normals, rows int64
    [n, 3] (x, y, crop)).  Read-only.  A crop of at most five rows has no tap above or below any of its pixels, so a pixel has a normal only
    where the zero-extended taps count: where its depth lies below the difference threshold.  dvc._values puts 1 mm at a tenth of the
    pixels; scene_image has no such pixel, which is why these crops are not scene_images."""
    crops, _, rows, _ = dvc.wide()
    scene = scene_image(dvc.WIDE_W, dvc.WIDE_H, np.random.default_rng(1))
    return crops, [np_normal_map(c) for c in crops], scene, np_normal_map(scene), rows


def padded(a, pitch):
    """[h, w, ...] -> [h, pitch, ...], zeros behind each row: a crop or its normals as the device stores them."""
    out = np.zeros((a.shape[0], pitch) + a.shape[2:], a.dtype)
    out[:, :a.shape[1]] = a
    return out


def packed(n):
    """int16 [..., 4] -> the uint64 element the device stores."""
    return np.ascontiguousarray(n).view(np.uint64)[..., 0]


def build_host_lib(directory):
    """g++ build of tests/cpp/normal_verify_host.cpp (the shared header with LMX_NV_HOST) as a library in `directory` -> ctypes handle."""
    so = os.path.join(str(directory), "libnvhost.so")
    subprocess.check_call(["g++"] + HOST_FLAGS + ["-fPIC", "-shared", "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.nv_host_table.argtypes = [vp]
    lib.nv_host_table.restype = None
    lib.nv_host_normal_map.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_int, vp]
    lib.nv_host_normal_map.restype = None
    lib.nv_host_angle_index.argtypes = [C.c_uint64, C.c_uint64]
    lib.nv_host_diff.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp]
    lib.nv_host_diff.restype = None
    lib.nv_host_diff_vectors.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp]
    lib.nv_host_diff_vectors.restype = None
    lib.nv_host_value.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_double]
    lib.nv_host_value.restype = C.c_double
    return lib


def host_map(lib, img, fx=FX, fy=FY, diff_t=DIFF_T, dist_t=DIST_T):
    """The header's normal map of a uint16 [h, w] image (rows may be strided) -> int16 [h, w, 4]."""
    h, w = img.shape
    out = np.zeros((h, w, 4), np.int16)
    lib.nv_host_normal_map(img.ctypes.data, w, h, img.strides[0] // 2, fx, fy, diff_t, dist_t, out.ctypes.data)
    return out
