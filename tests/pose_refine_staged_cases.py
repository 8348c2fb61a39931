"""Pose refinement under a schedule (csrc/lmx_pose_refine.hpp, SCHEDULE; refine_job_staged): the numpy restatement of the staged control --
written from the header's comment around the pass, solve and update of tests/pose_refine_cases.py -- and the builders of the cases
tests/test_pose_refine_staged_host.py and tests/test_gpu_pose_refine_staged.py run."""
import ctypes as C
import os
import subprocess

import numpy as np

import pose_refine_cases as prc
from pose_refine_cases import F8, LOST, MAX_ITERATIONS, CONVERGED, NO_OVERLAP, NONE, N_SUMS, _centroid, _llrint, _mat_point, _pass, _rms, _rotation_of, _solve, _update

STAGE_FIELDS = ("max_dist_mm", "eps_rot_rad", "eps_trans_mm", "max_iterations", "search_radius", "stride")


def make_stage(max_dist_mm=10.0, eps_rot_rad=1e-5, eps_trans_mm=1e-3, max_iterations=20, search_radius=1, stride=1):
    return dict(max_dist_mm=float(max_dist_mm), eps_rot_rad=float(eps_rot_rad), eps_trans_mm=float(eps_trans_mm), max_iterations=int(max_iterations),
                search_radius=int(search_radius), stride=int(stride))


def stage_of_params(P, stride=1):
    """The stage that repeats a parameter set."""
    return make_stage(P["max_dist_mm"], P["eps_rot_rad"], P["eps_trans_mm"], P["max_iterations"], P["search_radius"], stride)


def parse_schedule(text, **kw):
    """"stride:iterations:max_dist:radius,..." -> stages, the other fields from make_stage's defaults or kw."""
    out = []
    for part in text.split(","):
        g, it, dist, rad = part.split(":")
        out.append(make_stage(max_dist_mm=float(dist), max_iterations=int(it), search_radius=int(rad), stride=int(g), **kw))
    return out


def schedule_vector(stages):
    """The 6 doubles per stage tests/cpp/pose_refine_staged_host.cpp takes."""
    return np.asarray([[st[k] for k in STAGE_FIELDS] for st in stages], F8).reshape(-1)


def schedule_passes(stages):
    return sum(st["max_iterations"] for st in stages) + 1


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------

def np_refine_staged(P, stages, crop, rect_xy, scene, x, y):
    """-> (record: dict with the fields of lmx_pose_refine_t, sums: int64 [schedule_passes, 17], trace: per pass (stage, selected pixels))."""
    crop = np.asarray(crop, np.uint16)
    H, W = scene.shape
    sums = np.zeros((schedule_passes(stages), N_SUMS), np.int64)
    rec = dict(R=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], t_mm=[0.0, 0.0, 0.0], rms_first_mm=0.0, rms_last_mm=0.0, n_model=0, n_pairs_first=0,
               n_pairs_last=0, iterations=0, status=NONE, reserved=0)
    trace = []
    if crop.size == 0:
        rec["R"] = [0.0] * 9
        return rec, sums, trace
    # step 0: every crop pixel, whatever the strides
    i, j = np.nonzero(crop)
    i, j = i.astype(np.int64), j.astype(np.int64)
    tv = crop[i, j]
    rec["n_model"] = len(tv)
    rec["status"] = NO_OVERLAP
    X, Y = int(x) + j, int(y) + i
    met = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    s = np.zeros(len(tv), np.int64)
    s[met] = scene[Y[met], X[met]]
    pair = s != 0
    t64, u, v = tv.astype(np.int64)[pair], (rect_xy[0] + j)[pair], (rect_xy[1] + i)[pair]
    n0, St, Sut, Svt = int(pair.sum()), int(t64.sum()), int((u * t64).sum()), int((v * t64).sum())
    Ss, SXs, SYs = int(s[pair].sum()), int((X[pair] * s[pair]).sum()), int((Y[pair] * s[pair]).sum())
    if n0 < P["min_pairs"]:
        return rec, sums, trace
    m0 = _centroid(P["model"], n0, St, Sut, Svt)
    q0 = _centroid(P["scene"], n0, Ss, SXs, SYs)
    q = [1.0, 0.0, 0.0, 0.0]
    R = _rotation_of(q)
    t = [q0[k] - m0[k] for k in range(3)]
    row = 0
    stopped = False
    for si, st in enumerate(stages):
        last = si == len(stages) - 1
        Ps = dict(P, max_dist_mm=st["max_dist_mm"], eps_rot_rad=st["eps_rot_rad"], eps_trans_mm=st["eps_trans_mm"], search_radius=st["search_radius"])
        sel = (i % st["stride"] == 0) & (j % st["stride"] == 0)
        ii, jj, tt = i[sel], j[sel], tv[sel]
        rec["status"] = MAX_ITERATIONS
        final = last and st["max_iterations"] == 0
        k = 0
        while True:
            c = list(_mat_point(R, m0, t))
            Cc = [int(_llrint(F8(16.0 * c[m]))) for m in range(3)]
            a = _pass(Ps, R, t, Cc, rect_xy, ii, jj, tt, scene)
            sums[row] = a
            row += 1
            trace.append((si, len(tt)))
            if si == 0 and k == 0:
                rec["n_pairs_first"], rec["rms_first_mm"] = a[0], _rms(a)
            if final:
                rec["n_pairs_last"], rec["rms_last_mm"] = a[0], _rms(a)
                stopped = True
                break
            if a[0] < P["min_pairs"]:
                rec["status"], rec["n_pairs_last"], rec["rms_last_mm"] = LOST, a[0], _rms(a)
                stopped = True
                break
            w, v = _solve(a)
            q, t, conv = _update(Ps, w, v, c, q, t)
            R = _rotation_of(q)
            rec["iterations"] += 1
            if conv:
                rec["status"] = CONVERGED
            k += 1
            done = conv or k >= st["max_iterations"]
            if last:
                final = done
            elif done:
                break          # no measuring pass: the next stage's pass 0 runs under this q, R, t
        if stopped:
            rec["reserved"] = si
            break
    rec["R"], rec["t_mm"] = [float(v) for v in R], [float(v) for v in t]
    return rec, sums, trace


# ---- the CPU build of the header ------------------------------------------------------------------------------------------------------------

HOST_SRC = os.path.join(prc.ROOT, "tests", "cpp", "pose_refine_staged_host.cpp")
HOST_FLAGS = prc.HOST_FLAGS


def build_host(directory):
    so = os.path.join(str(directory), "libprshost.so")
    subprocess.check_call(["g++"] + HOST_FLAGS + ["-fPIC", "-shared", "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.prs_host_pitch.argtypes = [C.c_int]
    lib.prs_host_check_schedule.argtypes = [vp, C.c_int]
    lib.prs_host_refine.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]
    lib.prs_host_refine_plain.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    return lib


def _padded(lib, crop):
    crop = np.asarray(crop, np.uint16)
    h, w = crop.shape
    pitch = lib.prs_host_pitch(w) if w else 0
    pad = np.zeros((h, pitch), np.uint16)
    pad[:, :w] = crop
    return pad, w, h, pitch


def host_refine_staged(lib, P, stages, crop, rect_xy, scene, x, y, dtype):
    """The header's refine_job_staged on one job -> (POSE_REFINE_DTYPE element array [1], sums int64 [schedule_passes, 17])."""
    pad, w, h, pitch = _padded(lib, crop)
    scene = np.ascontiguousarray(scene, np.uint16)
    rec = np.zeros(1, dtype)
    assert lib.prs_host_record_bytes() == dtype.itemsize
    sums = np.zeros((schedule_passes(stages), N_SUMS), np.int64)
    v, s = prc.params_vector(P), schedule_vector(stages)
    rc = lib.prs_host_refine(pad.ctypes.data, w, h, pitch, int(rect_xy[0]), int(rect_xy[1]), scene.ctypes.data, scene.shape[1], scene.shape[0], scene.shape[1],
                             int(x), int(y), v.ctypes.data, s.ctypes.data, len(stages), rec.ctypes.data, sums.ctypes.data)
    assert rc == 0, "the parameters or the schedule were refused (%d)" % rc
    return rec, sums


def host_refine_plain(lib, P, crop, rect_xy, scene, x, y, dtype, as_single_stage=False):
    """refine_job from the same build, or refine_job_staged under single_stage(P)."""
    pad, w, h, pitch = _padded(lib, crop)
    scene = np.ascontiguousarray(scene, np.uint16)
    rec = np.zeros(1, dtype)
    sums = np.zeros((P["max_iterations"] + 1, N_SUMS), np.int64)
    v = prc.params_vector(P)
    rc = lib.prs_host_refine_plain(pad.ctypes.data, w, h, pitch, int(rect_xy[0]), int(rect_xy[1]), scene.ctypes.data, scene.shape[1], scene.shape[0], scene.shape[1],
                                   int(x), int(y), v.ctypes.data, int(as_single_stage), rec.ctypes.data, sums.ctypes.data)
    assert rc == 0
    return rec, sums


def check_schedule(lib, stages):
    """True: the header admits the schedule."""
    s = schedule_vector(stages) if stages else np.zeros(6, F8)
    return lib.prs_host_check_schedule(s.ctypes.data, len(stages)) == 0


# ---- constructed cases on the 96 x 80 scenes of pose_refine_cases -----------------------------------------------------------------------------

class StagedJob:
    """expect: dict of record fields the case is about (status, reserved, iterations), or None."""
    def __init__(self, name, crop, rect_xy, x, y, P, stages, scene="plain", expect=None):
        self.name, self.crop, self.rect_xy, self.x, self.y, self.P, self.stages, self.scene, self.expect = name, crop, rect_xy, x, y, P, stages, scene, expect


WIDE_AT = (-452, 30)   # the 530 x 3 crop: columns 452 .. 529 of it meet the scene, the rest hangs off its left side


def staged_crops():
    """name -> (crop, rect_xy, x, y).  530 x 3: 67 16-byte vectors a row, more than a wave's 64 lanes."""
    out = {}
    for (w, h) in ((3, 3), (9, 1), (8, 8), (33, 37)):
        c, r = prc.make_crop(w, h, (30, 20), drop=0.0 if w * h < 20 else 0.1)
        out["%dx%d" % (w, h)] = (c, r, 30, 20)
    c, r = prc.make_crop(70, 5, (10, 20))
    out["70x5"] = (c, r, 10, 20)
    c, r = prc.make_crop(530, 3, WIDE_AT)
    out["530x3"] = (c, r, WIDE_AT[0], WIDE_AT[1])
    return out


def constructed_jobs():
    base = dict(max_dist_mm=12.0, max_iterations=6, min_pairs=3, search_radius=1)
    P = lambda **kw: prc.make_params(prc.CAM, prc.CAM, **dict(base, **kw))
    St = lambda **kw: make_stage(**dict(dict(max_dist_mm=12.0, max_iterations=6), **kw))
    crops = staged_crops()
    jobs = []
    one_pixel = {("3x3", 8), ("8x8", 8), ("3x3", 4)}      # the lattice holds pixel (0, 0) alone: below min_pairs in pass 0 of stage 0
    for name, (c, r, x, y) in crops.items():
        for g in (2, 4, 8):
            expect = dict(status=LOST, reserved=0, iterations=0) if (name, g) in one_pixel else None
            jobs.append(StagedJob("crop_%s_stride_%d" % (name, g), c, r, x, y, P(), [St(stride=g), St(max_iterations=3)], expect=expect))
    c, r, x, y = crops["33x37"]
    jobs.append(StagedJob("four_stages", c, r, x, y, P(), [St(stride=8, search_radius=2), St(stride=4, search_radius=2), St(stride=2), St(max_iterations=2)],
                          scene="holes"))
    for rad in (0, 2):
        jobs.append(StagedJob("coarse_radius_%d" % rad, c, r, x, y, P(), [St(stride=4, search_radius=rad), St(max_iterations=3)], scene="holes"))
        cw, rw, xw, yw = crops["530x3"]
        jobs.append(StagedJob("wide_coarse_radius_%d" % rad, cw, rw, xw, yw, P(), [St(stride=2, search_radius=rad), St(max_iterations=3)], scene="holes"))
    jobs.append(StagedJob("lost_in_stage_1", c, r, x, y, P(min_pairs=27), [St(stride=2, max_iterations=4), St(max_dist_mm=0.05, search_radius=0)], scene="holes",
                          expect=dict(status=LOST, reserved=1, iterations=4)))
    eps = dict(eps_rot_rad=1e-3, eps_trans_mm=0.1, max_iterations=64)
    jobs.append(StagedJob("converged_in_stage_0", c, r, x, y, P(), [St(stride=2, **eps), St(**eps)], expect=dict(status=CONVERGED, reserved=1)))
    return jobs


def scenes():
    return prc.scenes()


GT_SCHEDULES = ("4:20:10:1,1:3:10:1", "8:20:20:1,2:10:10:1,1:2:10:1", "4:20:10:1,1:0:10:1")
