"""Pose verification (csrc/lmx_pose_verify.hpp): the numpy restatement of the header's opening comment -- written from that comment, with
Python integers for the counts and float64 arrays in the written order; the points, poses and ticks are those of the pose refinement, so
their restatement is the one of tests/pose_refine_cases.py -- and the builders of the cases tests/test_pose_verify_host.py and
tests/test_gpu_pose_verify.py run."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

import pose_refine_cases as prc
from pose_refine_cases import CAM, SCENE_H, SCENE_W

NONE, OK, EMPTY, GRID_TOO_LARGE = range(4)
MAX_CELLS = 1 << 18
F8 = np.float64
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def make_params(model=CAM, scene=CAM, voxel_mm=4.0, roi_margin=8):
    return dict(model=tuple(float(v) for v in model), scene=tuple(float(v) for v in scene), voxel_mm=float(voxel_mm), roi_margin=int(roi_margin))


def params_vector(P):
    """The 10 doubles tests/cpp/pose_verify_host.cpp takes."""
    return np.asarray(P["model"] + P["scene"] + (P["voxel_mm"], P["roi_margin"]), F8)


def verify_kwargs(P):
    """The keyword arguments of DepthTemplates.verify_poses."""
    return dict(model_camera=P["model"], scene_camera=P["scene"], voxel_mm=P["voxel_mm"], roi_margin=P["roi_margin"])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------

def _ticks(a):
    return np.rint(16.0 * np.asarray(a, F8)).astype(np.int64)


def np_model_points(P, crop, rect_xy, R, t):
    """The tested model points -> (n_model, keys int64 [n_tested, 3], xr, yr int64 [n_tested], ticks int64 [n_tested, 3])."""
    crop = np.asarray(crop, np.uint16)
    vt = int(np.rint(F8(16.0 * P["voxel_mm"])))
    i, j = np.nonzero(crop)
    i, j = i.astype(np.int64), j.astype(np.int64)
    M = prc._back(P["model"], rect_xy[0] + j, rect_xy[1] + i, crop[i, j])
    fx, fy, cx, cy = P["scene"]
    lim = 2.0 ** 20
    with np.errstate(all="ignore"):
        p = prc._mat_point([F8(v) for v in R], M, [F8(v) for v in t])
        ok = (p[2] >= 1.0) & (np.abs(p[0]) <= lim) & (np.abs(p[1]) <= lim) & (np.abs(p[2]) <= lim)
        xr = np.rint((p[0] * fx) / p[2] + cx)
        yr = np.rint((p[1] * fy) / p[2] + cy)
        ok &= (np.abs(xr) <= lim) & (np.abs(yr) <= lim)
    T = np.stack([_ticks(c[ok]) for c in p], 1) if ok.any() else np.zeros((0, 3), np.int64)
    return len(i), T // vt, xr[ok].astype(np.int64), yr[ok].astype(np.int64), T


def np_verify(P, crop, rect_xy, scene, R, t):
    """-> record: dict with the fields of lmx_pose_verify_t."""
    rec = dict(rate=0.0, n_model=0, n_tested=0, n_occupied=0, n_scene=0, cells=0, status=NONE, roi=[0, 0, 0, 0])
    crop = np.asarray(crop, np.uint16)
    if crop.size == 0:
        return rec
    H, W = scene.shape
    vt = int(np.rint(F8(16.0 * P["voxel_mm"])))
    n_model, K, xr, yr, _ = np_model_points(P, crop, rect_xy, R, t)
    rec["n_model"], rec["n_tested"], rec["status"] = n_model, len(K), EMPTY
    if len(K) == 0:
        return rec
    lo, hi = K.min(0), K.max(0)
    dims = [int(hi[k]) - int(lo[k]) + 1 for k in range(3)]
    cells = dims[0] * dims[1] * dims[2]
    rec["cells"] = min(cells, 2 ** 31 - 1)
    m = P["roi_margin"]
    x0, x1 = max(int(xr.min()) - m, 0), min(int(xr.max()) + m, W - 1)
    y0, y1 = max(int(yr.min()) - m, 0), min(int(yr.max()) + m, H - 1)
    some = x1 >= x0 and y1 >= y0
    rec["roi"] = [x0, y0, x1 - x0 + 1, y1 - y0 + 1] if some else [0, 0, 0, 0]
    rec["status"] = GRID_TOO_LARGE
    if cells > MAX_CELLS:
        return rec
    rec["status"] = OK
    marked = set()
    if some:
        Y, X = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        X, Y = X.reshape(-1).astype(np.int64), Y.reshape(-1).astype(np.int64)
        s = scene[Y, X]
        X, Y, s = X[s != 0], Y[s != 0], s[s != 0]
        Q = prc._back(P["scene"], X, Y, s)
        near = (np.abs(Q[0]) <= 2.0 ** 21) & (np.abs(Q[1]) <= 2.0 ** 21)
        KQ = np.stack([_ticks(c[near]) for c in Q], 1) // vt
        inside = ((KQ >= lo) & (KQ <= hi)).all(1)
        rec["n_scene"] = int(inside.sum())
        marked = set(map(tuple, KQ[inside].tolist()))
    rec["n_occupied"] = sum(1 for k in K.tolist() if tuple(k) in marked)
    rec["rate"] = float(rec["n_occupied"]) / float(n_model) if n_model > 0 else 0.0
    return rec


def np_keep(records, thresh):
    """The erase rule, record by record."""
    return np.asarray([bool(r["status"] == OK and not (r["rate"] < thresh)) for r in records], bool)


def record_array(rec, dtype):
    """A restatement record as one POSE_VERIFY_DTYPE element (for byte comparisons)."""
    out = np.zeros(1, dtype)
    for k in dtype.names:
        out[k][0] = rec[k]
    return out


# ---- the CPU build of the header ------------------------------------------------------------------------------------------------------------

HOST_SRC = os.path.join(prc.ROOT, "tests", "cpp", "pose_verify_host.cpp")
HOST_FLAGS = prc.HOST_FLAGS


def build_host(directory, opt=None):
    so = os.path.join(str(directory), "libpvhost.so")
    subprocess.check_call(["g++"] + HOST_FLAGS + ([opt] if opt else []) + ["-fPIC", "-shared", "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.pv_host_pitch.argtypes = [C.c_int]
    lib.pv_host_verify.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, vp]
    lib.pv_host_verify_batch.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]
    lib.pv_host_keep.argtypes = [vp, C.c_int, C.c_double, vp]
    lib.pv_host_keep.restype = None
    return lib


def pose_vector(R, t):
    return np.asarray(list(R) + list(t), F8)


def host_verify_rc(lib, P, crop, rect_xy, scene, R, t, dtype):
    """The header's verify_job on one job -> (return code, POSE_VERIFY_DTYPE element array [1])."""
    crop = np.asarray(crop, np.uint16)
    h, w = crop.shape
    pitch = lib.pv_host_pitch(w) if w else 0
    pad = np.zeros((h, pitch), np.uint16)
    pad[:, :w] = crop
    scene = np.ascontiguousarray(scene, np.uint16)
    rec = np.zeros(1, dtype)
    assert lib.pv_host_record_bytes() == dtype.itemsize and lib.pv_host_max_cells() == MAX_CELLS
    v, pose = params_vector(P), pose_vector(R, t)
    rc = lib.pv_host_verify(pad.ctypes.data, w, h, pitch, int(rect_xy[0]), int(rect_xy[1]), scene.ctypes.data, scene.shape[1], scene.shape[0], scene.shape[1],
                            pose.ctypes.data, v.ctypes.data, rec.ctypes.data)
    return rc, rec


def host_verify(lib, P, crop, rect_xy, scene, R, t, dtype):
    rc, rec = host_verify_rc(lib, P, crop, rect_xy, scene, R, t, dtype)
    assert rc == 0, "the parameters or the pose were refused"
    return rec


# ---- constructed cases: the 96 x 80 scene and the cameras of pose_refine_cases ---------------------------------------------------------------

BACKGROUND = 900   # mm: behind every object point (the surface stays below 710) by far more than a voxel


def make_crop(w, h, at, drop=0.1, seed=1):
    """A w x h crop of pose_refine_cases.surface as rendered at `at` -> (crop, rect_xy = at)."""
    c, r = prc.make_crop(w, h, at, shift=(0.0, 0.0), dz=0.0, drop=drop if w * h >= 20 else 0.0, seed=seed)
    return c, r


def paste(crop, rect_xy, background=BACKGROUND):
    """The scene that holds the crop's object pixels at its own rect, in front of a plane; what falls outside the image is cut off."""
    s = np.full((SCENE_H, SCENE_W), background, np.uint16)
    h, w = crop.shape
    for i in range(h):
        for j in range(w):
            X, Y = rect_xy[0] + j, rect_xy[1] + i
            if crop[i, j] != 0 and 0 <= X < SCENE_W and 0 <= Y < SCENE_H:
                s[Y, X] = crop[i, j]
    return s


def rotation_y(deg):
    a = math.radians(deg)
    return (math.cos(a), 0.0, math.sin(a), 0.0, 1.0, 0.0, -math.sin(a), 0.0, math.cos(a))


def splat(P, crop, rect_xy, R, t, background=BACKGROUND):
    """The scene a camera sees of the crop's points moved by (R, t): nearest depth per pixel in front of a plane."""
    i, j = np.nonzero(crop)
    M = prc._back(P["model"], rect_xy[0] + j.astype(np.int64), rect_xy[1] + i.astype(np.int64), crop[i, j])
    p = prc._mat_point([F8(v) for v in R], M, [F8(v) for v in t])
    fx, fy, cx, cy = P["scene"]
    s = np.full((SCENE_H, SCENE_W), background, np.uint16)
    for x, y, z in zip(np.rint(p[0] * fx / p[2] + cx).astype(int), np.rint(p[1] * fy / p[2] + cy).astype(int), np.rint(p[2]).astype(int)):
        if 0 <= x < SCENE_W and 0 <= y < SCENE_H and z < s[y, x]:
            s[y, x] = z
    return s


class Job:
    def __init__(self, name, crop, rect_xy, scene, P, R=IDENTITY, t=(0.0, 0.0, 0.0), expect=None):
        self.name, self.crop, self.rect_xy, self.scene, self.P, self.R, self.t, self.expect = name, crop, rect_xy, scene, P, tuple(R), tuple(t), expect


# voxel_mm 0.25: crops of the surface at (40, 30) whose grids lie just below and just above the cap (found with np_verify; the tests assert it)
BELOW_CAP, ABOVE_CAP = (14, 11), (15, 11)
TURN_DEG = 10.0


@functools.lru_cache(maxsize=None)
def turned_case():
    """A 33 x 37 crop, the scene that shows it turned by TURN_DEG about the y axis through its centroid, and the pose np_refine finds from
    the crop's own position -> (crop, rect_xy, scene, refine record)."""
    P = make_params()
    c, r = make_crop(33, 37, (30, 20))
    i, j = np.nonzero(c)
    M = prc._back(P["model"], r[0] + j.astype(np.int64), r[1] + i.astype(np.int64), c[i, j])
    g = np.asarray([float(np.mean(v)) for v in M])
    R = np.asarray(rotation_y(TURN_DEG)).reshape(3, 3)
    t = g - R @ g
    scene = splat(P, c, r, R.reshape(9), t)
    PR = prc.make_params(CAM, CAM, max_dist_mm=40.0, max_iterations=40, min_pairs=16, search_radius=2)
    rec, _ = prc.np_refine(PR, c, r, scene, r[0], r[1])
    return c, r, scene, rec


def constructed_jobs():
    """Single jobs, each the smallest shape at which something can go wrong; `expect` names what the case is about."""
    P = make_params
    jobs = []
    for (w, h) in ((1, 1), (17, 1), (33, 37), (70, 70)):
        at = (10, 5) if w == 70 else (30, 20)
        c, r = make_crop(w, h, at)
        jobs.append(Job("identity_%dx%d" % (w, h), c, r, paste(c, r), P(), expect="all"))
    c, r = make_crop(33, 37, (30, 20))
    behind = paste(np.where(c != 0, int(c.max()) + 50, 0).astype(np.uint16), r)
    jobs.append(Job("plane_behind", c, r, behind, P(), expect="none"))
    occluded = paste(c, r)
    cover = np.zeros_like(c)
    cover[:, :16] = int(c[c != 0].min()) - 50
    occluded[r[1]:r[1] + 37, r[0]:r[0] + 16] = cover[:, :16]
    jobs.append(Job("left_half_occluded", c, r, occluded, P(), expect="part"))
    cs, rs = make_crop(33, 37, (32, 22))                     # the principal point (48, 40) lies inside
    jobs.append(Job("straddles_principal_point", cs, rs, paste(cs, rs), P(), expect="all"))
    for name, at in (("roi_partly_outside", (-10, -12)), ("roi_partly_outside_far_corner", (SCENE_W - 20, SCENE_H - 15))):
        jobs.append(Job(name, c, at, paste(c, at), P(), expect="clipped"))
    jobs.append(Job("roi_wholly_outside", c, (120, 10), paste(c, r), P(), expect="outside"))
    jobs.append(Job("roi_wholly_above", c, (30, -60), paste(c, r), P(), expect="outside"))
    shift = (3.0 * 650.0 / 400.0, 0.0, 0.0)                  # about 3 pixels to the right at the object's depth
    for m in (0, 8):
        jobs.append(Job("shifted_margin_%d" % m, c, r, paste(c, r), P(voxel_mm=16.0, roi_margin=m), t=shift))
    ct, rt, turned, rec = turned_case()
    jobs.append(Job("turned_by_refine", ct, rt, turned, P(), R=rec["R"], t=rec["t_mm"]))
    jobs.append(Job("turned_identity", ct, rt, turned, P()))      # the same scene under the pose that was not refined
    jobs.append(Job("behind_camera", c, r, paste(c, r), P(), R=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0), expect=EMPTY))
    for name, (w, h) in (("cap_below", BELOW_CAP), ("cap_above", ABOVE_CAP)):
        cc, rc = make_crop(w, h, (40, 30), drop=0.0)
        jobs.append(Job(name, cc, rc, paste(cc, rc), P(voxel_mm=0.25), expect=GRID_TOO_LARGE if name == "cap_above" else "all"))
    jobs.append(Job("voxel_64", c, r, paste(c, r), P(voxel_mm=64.0), expect="all"))
    jobs.append(Job("voxel_64_behind", c, r, behind, P(voxel_mm=64.0, roi_margin=0)))
    return jobs
