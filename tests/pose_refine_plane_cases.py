"""Point-to-plane pose refinement (csrc/lmx_pose_refine.hpp, PLANE; refine_job_plane, solve_plane): the numpy restatement of that paragraph --
written from the header's comment, Python integers for the sums and float64 scalars in the written order, sharing no code with the header --
and the builders of the cases tests/test_pose_refine_plane_host.py and tests/test_gpu_pose_refine_plane.py run.  The scenes and crops are
those of pose_refine_cases and pose_refine_staged_cases; the scene normals are normal_verify_cases.np_normal_map."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

import normal_verify_cases as nvc
import pose_refine_cases as prc
import pose_refine_staged_cases as psc
from pose_refine_cases import F8, LOST, MAX_ITERATIONS, CONVERGED, NONE, NO_OVERLAP, N_SUMS, _back, _centroid, _llrint, _mat_point, _rms, _rotation_of, _solve, _update

N_PLANE = 29
NORMAL_FX = NORMAL_FY = 400.0          # the focal lengths the constructed scenes' normals are computed with
DIFF_T, DIST_T = 50, 2000
POINT, FEW, FALLBACK, PLANE = "point", "few", "fallback", "plane"   # which way a step went


def scene_normals(scene, fx=NORMAL_FX, fy=NORMAL_FY, difference_threshold=DIFF_T, distance_threshold=DIST_T):
    """int16 [H, W, 4] = (qx, qy, qz, valid): the stored normals of a scene, as lmx_depth_templates_enable_normals' parameters give them."""
    return nvc.np_normal_map(np.asarray(scene, np.uint16), fx=fx, fy=fy, difference_threshold=difference_threshold, distance_threshold=distance_threshold)


def packed(normals):
    """The same normals as the header's nv::Packed elements, uint64 [H, W]."""
    return np.ascontiguousarray(normals, np.int16).view(np.uint64).reshape(normals.shape[:2])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------

def _rs14(a):
    return (a + 8192) >> 14            # int64 arrays and Python integers both shift arithmetically


def _pass_plane(P, R, t, C, rect, i, j, tv, scene, normals):
    """PASS k with the candidate's pixel kept: -> (the 17 sums, the 29 plane sums), Python integers."""
    H, W = scene.shape
    dmax = int(_llrint(F8(16.0 * P["max_dist_mm"])))
    fx, fy, cx, cy = P["scene"]
    M = _back(P["model"], rect[0] + j, rect[1] + i, tv)
    with np.errstate(all="ignore"):
        p = _mat_point(R, M, t)
        lim = 2.0 ** 20
        ok = (p[2] >= 1.0) & (np.abs(p[0]) <= lim) & (np.abs(p[1]) <= lim) & (np.abs(p[2]) <= lim)
        xr = np.rint((p[0] * fx) / p[2] + cx)
        yr = np.rint((p[1] * fy) / p[2] + cy)
        ok &= (np.abs(xr) <= lim) & (np.abs(yr) <= lim)
    p = [c[ok] for c in p]
    X0, Y0 = xr[ok].astype(np.int64), yr[ok].astype(np.int64)
    Pt = [_llrint(16.0 * c) for c in p]
    n = len(X0)
    found = np.zeros(n, bool)
    best = np.zeros(n, np.int64)
    D = [np.zeros(n, np.int64) for _ in range(3)]
    bX, bY = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rad = P["search_radius"]
    for dy in range(-rad, rad + 1):
        for dx in range(-rad, rad + 1):
            X, Y = X0 + dx, Y0 + dy
            cand = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
            s = np.zeros(n, np.uint16)
            s[cand] = scene[Y[cand], X[cand]]
            cand &= s != 0
            Q = _back(P["scene"], X, Y, s)
            cand &= (np.abs(Q[0]) <= 2.0 ** 21) & (np.abs(Q[1]) <= 2.0 ** 21)
            Q = [np.where(cand, c, 0.0) for c in Q]
            d = [np.where(cand, _llrint(16.0 * Q[k]) - Pt[k], 0) for k in range(3)]
            cand &= (np.abs(d[0]) <= dmax) & (np.abs(d[1]) <= dmax) & (np.abs(d[2]) <= dmax)
            d = [np.where(cand, c, 0) for c in d]
            dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            take = cand & (~found | (dd < best))
            best = np.where(take, dd, best)
            D = [np.where(take, d[k], D[k]) for k in range(3)]
            bX, bY = np.where(take, X, bX), np.where(take, Y, bY)
            found |= take
    x, y, z = Pt[0] - C[0], Pt[1] - C[1], Pt[2] - C[2]
    big = 1 << 15
    acc = found & (best <= dmax * dmax) & (np.abs(x) <= big) & (np.abs(y) <= big) & (np.abs(z) <= big)
    x, y, z, best = x[acc], y[acc], z[acc], best[acc]
    Dx, Dy, Dz = D[0][acc], D[1][acc], D[2][acc]
    terms = [np.ones(len(x), np.int64), x, y, z, Dx, Dy, Dz, x * x, x * y, x * z, y * y, y * z, z * z, y * Dz - z * Dy, z * Dx - x * Dz, x * Dy - y * Dx, best]
    a = [int(np.sum(v, dtype=np.int64)) for v in terms]
    # the plane terms of the pairs whose scene pixel holds a valid normal
    N = normals[bY[acc], bX[acc]].astype(np.int64)
    v = N[:, 3] != 0
    x, y, z, Dx, Dy, Dz = x[v], y[v], z[v], Dx[v], Dy[v], Dz[v]
    Nx, Ny, Nz = N[v, 0], N[v, 1], N[v, 2]
    g = [_rs14(y * Nz - z * Ny), _rs14(z * Nx - x * Nz), _rs14(x * Ny - y * Nx), Nx, Ny, Nz]
    r = _rs14(Dx * Nx + Dy * Ny + Dz * Nz)
    pt = [np.ones(len(x), np.int64)] + [g[m] * g[k] for m in range(6) for k in range(m, 6)] + [g[m] * r for m in range(6)] + [r * r]
    pl = [int(np.sum(q, dtype=np.int64)) for q in pt]
    assert len(pl) == N_PLANE
    return a, pl


def _cholesky_step(A, b):
    """SOLVE's Cholesky, substitutions and acceptance test on a float system -> (accepted, w, v)."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0.0:
            return False, None, None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            e = A[i][j]
            for k in range(j):
                e = e - L[i][k] * L[j][k]
            L[i][j] = e / L[j][j]
    y, z = [0.0] * 6, [0.0] * 6
    for i in range(6):
        e = b[i]
        for k in range(i):
            e = e - L[i][k] * y[k]
        y[i] = e / L[i][i]
    for i in range(5, -1, -1):
        e = y[i]
        for k in range(i + 1, 6):
            e = e - L[k][i] * z[k]
        z[i] = e / L[i][i]
    w, v = z[:3], z[3:]
    ok = ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) <= 1.0 and ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) <= 2.0 ** 48
    return ok, w, v


def _solve_plane(a, pl, min_pairs, k):
    """-> (w, v, which way the step went)."""
    if pl[0] < min_pairs:
        return _solve(a) + (FEW,)
    n, sx, sy, sz = a[0], a[1], a[2], a[3]
    Ai = [[a[10] + a[12], -a[8], -a[9], 0, -sz, sy],
          [-a[8], a[7] + a[12], -a[11], sz, 0, -sx],
          [-a[9], -a[11], a[7] + a[10], -sy, sx, 0],
          [0, sz, -sy, n, 0, 0],
          [-sz, 0, sx, 0, n, 0],
          [sy, -sx, 0, 0, 0, n]]
    b_pt = [float(a[13]), float(a[14]), float(a[15]), float(a[4]), float(a[5]), float(a[6])]
    lam = 1.0 / float(1 << k)
    s = [1.0, 1.0, 1.0, 1.0 / 16384.0, 1.0 / 16384.0, 1.0 / 16384.0]
    A = [[0.0] * 6 for _ in range(6)]
    q = 1
    for i in range(6):
        for j in range(i, 6):
            G = (float(pl[q]) * s[i]) * s[j]
            q += 1
            A[i][j] = A[j][i] = G + lam * float(Ai[i][j])
    b = [float(pl[22 + i]) * s[i] + lam * b_pt[i] for i in range(6)]
    ok, w, v = _cholesky_step(A, b)
    if not ok:
        return _solve(a) + (FALLBACK,)
    return w, v, PLANE


def np_refine_plane(P, stages, shifts, crop, rect_xy, scene, normals, x, y):
    """stages: a schedule, or None for the parameters' own single stage; shifts: a point_shift per stage (missing ones are -1); normals: int16
    [H, W, 4].  -> (record dict, sums int64 [passes, 17], plane sums int64 [passes, 29], trace: per pass (stage, selected pixels, route or None))."""
    if not stages:
        stages = [psc.stage_of_params(P)]
    shifts = list(shifts or []) + [-1] * (4 - len(shifts or []))
    crop = np.asarray(crop, np.uint16)
    H, W = scene.shape
    rows = psc.schedule_passes(stages)
    sums, plane_sums = np.zeros((rows, N_SUMS), np.int64), np.zeros((rows, N_PLANE), np.int64)
    rec = dict(R=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], t_mm=[0.0, 0.0, 0.0], rms_first_mm=0.0, rms_last_mm=0.0, n_model=0, n_pairs_first=0,
               n_pairs_last=0, iterations=0, status=NONE, reserved=0)
    trace = []
    if crop.size == 0:
        rec["R"] = [0.0] * 9
        return rec, sums, plane_sums, trace
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
        return rec, sums, plane_sums, trace
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
            if shifts[si] >= 0:
                a, pl = _pass_plane(Ps, R, t, Cc, rect_xy, ii, jj, tt, scene, normals)
                plane_sums[row] = pl
            else:
                a, pl = prc._pass(Ps, R, t, Cc, rect_xy, ii, jj, tt, scene), None
            sums[row] = a
            row += 1
            if si == 0 and k == 0:
                rec["n_pairs_first"], rec["rms_first_mm"] = a[0], _rms(a)
            if final or a[0] < P["min_pairs"]:
                if not final:
                    rec["status"] = LOST
                rec["n_pairs_last"], rec["rms_last_mm"] = a[0], _rms(a)
                trace.append((si, len(tt), None))
                stopped = True
                break
            if pl is None:
                (w, v), route = _solve(a), POINT
            else:
                w, v, route = _solve_plane(a, pl, P["min_pairs"], shifts[si])
            trace.append((si, len(tt), route))
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
                break
        if stopped:
            rec["reserved"] = si
            break
    rec["R"], rec["t_mm"] = [float(v) for v in R], [float(v) for v in t]
    return rec, sums, plane_sums, trace


# ---- the CPU build of the header ------------------------------------------------------------------------------------------------------------

HOST_SRC = os.path.join(prc.ROOT, "tests", "cpp", "pose_refine_plane_host.cpp")
HOST_FLAGS = prc.HOST_FLAGS


def build_host(directory):
    so = os.path.join(str(directory), "libprphost.so")
    subprocess.check_call(["g++"] + HOST_FLAGS + ["-fPIC", "-shared", "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.prp_host_pitch.argtypes = [C.c_int]
    lib.prp_host_check_plane.argtypes = [vp, C.c_int]
    lib.prp_host_refine.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.prp_host_refine_point.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp, vp]
    return lib


def _padded(lib, crop):
    crop = np.asarray(crop, np.uint16)
    h, w = crop.shape
    pitch = lib.prp_host_pitch(w) if w else 0
    pad = np.zeros((h, pitch), np.uint16)
    pad[:, :w] = crop
    return pad, w, h, pitch


def host_refine_plane(lib, P, stages, shifts, crop, rect_xy, scene, normals, x, y, dtype):
    """The header's refine_job_plane on one job -> (POSE_REFINE_DTYPE element array [1], sums int64 [passes, 17], plane sums int64 [passes, 29])."""
    if not stages:
        stages = [psc.stage_of_params(P)]
    pad, w, h, pitch = _padded(lib, crop)
    scene = np.ascontiguousarray(scene, np.uint16)
    nrm = packed(normals) if normals is not None else None
    rec = np.zeros(1, dtype)
    assert lib.prp_host_record_bytes() == dtype.itemsize
    rows = psc.schedule_passes(stages)
    sums, plane_sums = np.zeros((rows, N_SUMS), np.int64), np.zeros((rows, N_PLANE), np.int64)
    v, s = prc.params_vector(P), psc.schedule_vector(stages)
    k = np.asarray(list(shifts or []) + [-1] * (4 - len(shifts or [])), np.int32)
    rc = lib.prp_host_refine(pad.ctypes.data, w, h, pitch, int(rect_xy[0]), int(rect_xy[1]), scene.ctypes.data, nrm.ctypes.data if nrm is not None else None,
                             scene.shape[1], scene.shape[0], scene.shape[1], int(x), int(y), v.ctypes.data, s.ctypes.data, len(stages), k.ctypes.data, rec.ctypes.data,
                             sums.ctypes.data, plane_sums.ctypes.data)
    assert rc == 0, "the parameters, the schedule or the shifts were refused (%d)" % rc
    return rec, sums, plane_sums


def host_refine_point(lib, P, crop, rect_xy, scene, x, y, dtype):
    """The point-to-point definition from the same build: refine_job, untouched by PLANE."""
    pad, w, h, pitch = _padded(lib, crop)
    scene = np.ascontiguousarray(scene, np.uint16)
    rec = np.zeros(1, dtype)
    sums = np.zeros((P["max_iterations"] + 1, N_SUMS), np.int64)
    v = prc.params_vector(P)
    rc = lib.prp_host_refine_point(pad.ctypes.data, w, h, pitch, int(rect_xy[0]), int(rect_xy[1]), scene.ctypes.data, scene.shape[1], scene.shape[0], scene.shape[1],
                                   int(x), int(y), v.ctypes.data, rec.ctypes.data, sums.ctypes.data)
    assert rc == 0
    return rec, sums


def check_plane(lib, shifts):
    """True: the header admits the point_shift list."""
    k = np.asarray(list(shifts) + [0], np.int32)
    return lib.prp_host_check_plane(k.ctypes.data, len(shifts)) == 0


# ---- constructed cases on the 96 x 80 scenes ---------------------------------------------------------------------------------------------------

class PlaneJob:
    """stages: a schedule or None (the parameters' single stage); shifts: per stage; normals: the key of scene_normal_maps()."""
    def __init__(self, name, crop, rect_xy, x, y, P, stages, shifts, scene="plain", normals=None):
        self.name, self.crop, self.rect_xy, self.x, self.y, self.P, self.stages, self.shifts, self.scene = name, crop, rect_xy, x, y, P, stages, shifts, scene
        self.normals = normals or scene


INVALID_DISTANCE_THRESHOLD = 100      # below every depth of the constructed scenes: no pixel has a valid normal
NEAR_DISTANCE_THRESHOLD = 630         # about a quarter of the pixels under the 33 x 37 crop lie nearer: 249 of its 1050 pairs have a valid normal
DISTANCE_THRESHOLDS = {"": DIST_T, "/invalid": INVALID_DISTANCE_THRESHOLD, "/near": NEAR_DISTANCE_THRESHOLD}   # by the suffix of a normal map's name


def scenes():
    return prc.scenes()


@functools.lru_cache(maxsize=None)
def scene_normal_maps():
    """name -> int16 [H, W, 4]: each scene's normals, and "<scene>/invalid", "<scene>/near": the maps of the smaller distance thresholds."""
    out = {}
    for name, s in scenes().items():
        for suffix, threshold in DISTANCE_THRESHOLDS.items():
            out[name + suffix] = scene_normals(s, distance_threshold=threshold)
        assert not out[name + "/invalid"][..., 3].any()
    return out


def constructed_jobs():
    base = dict(max_dist_mm=12.0, max_iterations=4, min_pairs=3, search_radius=1)
    P = lambda **kw: prc.make_params(prc.CAM, prc.CAM, **dict(base, **kw))
    St = lambda **kw: psc.make_stage(**dict(dict(max_dist_mm=12.0, max_iterations=3), **kw))
    crops = psc.staged_crops()
    jobs = []
    for name in ("3x3", "9x1", "8x8", "33x37"):
        c, r, x, y = crops[name]
        for k in ((8,) if name != "33x37" else (0, 4, 8, 20)):
            jobs.append(PlaneJob("crop_%s_shift_%d" % (name, k), c, r, x, y, P(), None, [k]))
    for rad in (0, 1, 2):
        cb, rb = prc.make_crop(20, 12, (1, 1), shift=(-1.6, -1.3))
        jobs.append(PlaneJob("radius_%d_border" % rad, cb, rb, 0, 0, P(search_radius=rad), None, [8], scene="holes"))
        cb, rb = prc.make_crop(20, 12, (prc.SCENE_W - 21, prc.SCENE_H - 13), shift=(1.6, 1.4), seed=3)
        jobs.append(PlaneJob("radius_%d_far_border" % rad, cb, rb, prc.SCENE_W - 20, prc.SCENE_H - 12, P(search_radius=rad), None, [4], scene="sparse"))
    c, r, x, y = crops["33x37"]
    jobs.append(PlaneJob("holes", c, r, x, y, P(), None, [8], scene="holes"))
    jobs.append(PlaneJob("sparse", c, r, x, y, P(), None, [8], scene="sparse"))
    # min_pairs between the count of pairs with a valid normal and the pairs' count: the n_plane < min_pairs way
    jobs.append(PlaneJob("few_normals", c, r, x, y, P(min_pairs=300), None, [8], scene="holes", normals="holes/near"))
    jobs.append(PlaneJob("all_invalid", c, r, x, y, P(), None, [8], scene="holes", normals="holes/invalid"))
    # a flat crop on the fronto-parallel plane at the smallest point weight: the plane part has rank 3, the point term carries the rest
    flat = np.full((9, 14), 705, np.uint16)
    jobs.append(PlaneJob("flat_shift_20", flat, (20, 40), 20, 40, P(search_radius=0, max_iterations=3), None, [20], scene="plane"))
    # one row on that plane: every P'.y and P'.z is 0 and no weight makes the system definite; back to SOLVE and its translation-only step
    row = np.full((1, 24), 705, np.uint16)
    jobs.append(PlaneJob("singular_row", row, (20, 40), 20, 40, P(search_radius=0, max_iterations=3), None, [8], scene="plane"))
    jobs.append(PlaneJob("coarse_plane_fine_point", c, r, x, y, P(), [St(stride=4, search_radius=2), St(max_iterations=2)], [8, -1], scene="holes"))
    jobs.append(PlaneJob("point_then_plane", c, r, x, y, P(), [St(stride=2), St(max_iterations=2)], [-1, 4], scene="holes"))
    jobs.append(PlaneJob("four_alternating", c, r, x, y, P(), [St(stride=8, search_radius=2, max_iterations=2), St(stride=4, max_iterations=2), St(stride=2, max_iterations=2),
                                                            St(max_iterations=2)], [8, -1, 0, -1]))
    return jobs


# ---- the ground-truth case ---------------------------------------------------------------------------------------------------------------------

GT_SHIFT = 8
GT_ITERATIONS = 5


@functools.lru_cache(maxsize=None)
def ground_truth_normals():
    g = prc.ground_truth_case()
    return scene_normals(g["scene"], fx=prc.GT_F, fy=prc.GT_F)


def ground_truth_placements():
    bx, by = prc.ground_truth_case()["rect_b"][:2]
    return ((bx, by), (bx + 1, by), (bx, by + 1))
