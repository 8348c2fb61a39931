"""The rough pose stage (csrc/lmx_rough_pose.hpp, lmx_rough_pose_chain_on): a restatement of the header's opening comment in float64 scalar
operations in the written order (np_rough), the CPU build of the header (tests/cpp/rough_pose_host.cpp), view tables and exported lists
(on top of pose_chain_cases.build_lists) built for each rule, and the small meshes the GPU test renders.  tests/test_rough_pose_host.py and
tests/test_gpu_rough_pose.py run the same cases: the device must equal the CPU build byte for byte, and the CPU build this restatement."""
import os
import subprocess

import numpy as np

import pose_chain_cases as pcc
import pose_refine_cases as prc
from linemod_pose_estimation_amd import ROUGH_POSE_DTYPE

DEAD, BROKEN, NO_JOB_BOUNDS, NO_JOB_CLASS, JOB = range(5)          # pc::State
NONE, OK, TOO_MANY_GROUPS, DEGENERATE, INVALID_VIEW, WINDOW_TOO_LARGE, EMPTY = range(7)
FLAG_CUT, FLAG_BOUNDS, FLAG_POSE, FLAG_ROUGH = 1, 2, 4, 8
MAX_GROUPS = 512
MAX_MEAN = 1 << 17
FILL = 0x5a5a5a5a
HOST_SRC = os.path.join(prc.ROOT, "tests", "cpp", "rough_pose_host.cpp")
f8 = np.float64


# ---- the definition, restated ------------------------------------------------------------------------------------------------------------------

def quat_of(R):
    """Eigen 3's matrix-to-quaternion -> (x, y, z, w)"""
    R = [f8(v) for v in np.asarray(R, f8).reshape(9)]
    q = [f8(0)] * 4
    t = (R[0] + R[4]) + R[8]
    if t > 0:
        s = np.sqrt(t + f8(1))
        h = f8(0.5) / s
        return [(R[7] - R[5]) * h, (R[2] - R[6]) * h, (R[3] - R[1]) * h, f8(0.5) * s]
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[i * 4]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    s = np.sqrt(((R[i * 4] - R[j * 4]) - R[k * 4]) + f8(1))
    h = f8(0.5) / s
    q[i] = f8(0.5) * s
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * h
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * h
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * h
    return q


def trace_dot(A, B):
    """A [9], B [n, 9] -> [n]: the sum of the nine products, left to right (numpy's elementwise operations round as the scalar ones)"""
    B = np.asarray(B, f8).reshape(-1, 9)
    tr = B[:, 0] * f8(A[0])
    for k in range(1, 9):
        tr = tr + B[:, k] * f8(A[k])
    return tr


def rot_of_quat(x, y, z, w):
    tx, ty, tz = f8(2) * x, f8(2) * y, f8(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f8(1)
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


# libstdc++'s std::sort as csrc/lmx_sort_emul.hpp restates it, on a list of indices

def _linear_insert(a, last, less):
    val = a[last]
    nxt = last - 1
    while less(val, a[nxt]):
        a[last] = a[nxt]
        last = nxt
        nxt -= 1
    a[last] = val


def _insertion(a, first, last, less):
    for i in range(first + 1, last):
        if less(a[i], a[first]):
            val = a[i]
            a[first + 1:i + 1] = a[first:i]
            a[first] = val
        else:
            _linear_insert(a, i, less)


def _adjust_heap(a, first, hole, n, value, less):
    top = hole
    second = hole
    while second < (n - 1) // 2:
        second = 2 * (second + 1)
        if less(a[first + second], a[first + second - 1]):
            second -= 1
        a[first + hole] = a[first + second]
        hole = second
    if n % 2 == 0 and second == (n - 2) // 2:
        second = 2 * (second + 1)
        a[first + hole] = a[first + second - 1]
        hole = second - 1
    parent = (hole - 1) // 2
    while hole > top and less(a[first + parent], value):
        a[first + hole] = a[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    a[first + hole] = value


def _heap_sort(a, first, last, less):
    n = last - first
    if n >= 2:
        parent = (n - 2) // 2
        while True:
            _adjust_heap(a, first, parent, n, a[first + parent], less)
            if parent == 0:
                break
            parent -= 1
    while last - first > 1:
        last -= 1
        value = a[last]
        a[last] = a[first]
        _adjust_heap(a, first, 0, last - first, value, less)


def emul_sort(a, less):
    n = len(a)
    if n == 0:
        return a

    def swap(p, q):
        a[p], a[q] = a[q], a[p]
    stack = [(0, n, 2 * (n.bit_length() - 1))]
    while stack:
        first, last, depth = stack.pop()
        while last - first > 16:
            if depth == 0:
                _heap_sort(a, first, last, less)
                break
            depth -= 1
            mid = first + (last - first) // 2
            x, y, z = first + 1, mid, last - 1
            if less(a[x], a[y]):
                swap(first, y if less(a[y], a[z]) else (z if less(a[x], a[z]) else x))
            elif less(a[x], a[z]):
                swap(first, x)
            elif less(a[y], a[z]):
                swap(first, z)
            else:
                swap(first, y)
            lo, hi = first + 1, last
            while True:
                while less(a[lo], a[first]):
                    lo += 1
                hi -= 1
                while less(a[first], a[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                swap(lo, hi)
                lo += 1
            stack.append((lo, last, depth))
            last = lo
    if n > 16:
        _insertion(a, 0, 16, less)
        for i in range(16, n):
            _linear_insert(a, i, less)
    else:
        _insertion(a, 0, n, less)
    return a


def winning_group(sizes):
    return emul_sort(list(range(len(sizes))), lambda i, j: sizes[i] > sizes[j])[0]


class Views:
    """The view table: R [n, 9], distance, D, ori_dist [n]"""

    def __init__(self, R, distance, D=None, ori_dist=None):
        self.R = np.ascontiguousarray(R, f8).reshape(-1, 9)
        n = len(self.R)
        self.distance = np.broadcast_to(np.asarray(distance, f8), (n,)).copy()
        self.D = np.zeros(n) if D is None else np.asarray(D, f8).copy()
        self.ori_dist = np.zeros(n) if ori_dist is None else np.asarray(ori_dist, f8).copy()
        self.q = np.asarray([quat_of(r) for r in self.R], f8)

    def __len__(self):
        return len(self.R)

    def pairs(self):
        return [(r.reshape(3, 3), float(d)) for r, d in zip(self.R, self.distance)]


def _frame_of(L, k, caps):
    """pc::frame_claims / frame_state / cluster_ok -> (state, flags, frame)"""
    info = L.frame_info.astype(np.int64)
    claims = [f for f in range(len(info)) if info[f, 3] > 0 and info[f, 2] <= k < info[f, 2] + info[f, 3]]
    if not claims:
        return DEAD, 0, -1
    if len(claims) > 1:
        return BROKEN, FLAG_BOUNDS, -1
    f = claims[0]
    mb, mc, cb, cc, eb, ec, status = (int(v) for v in info[f, :7])
    if min(mb, mc, cb, cc, eb, ec) < 0:
        return BROKEN, FLAG_BOUNDS, -1
    if int(L.header[1]) & 1:
        return DEAD, FLAG_CUT, -1
    if status != 0:
        return DEAD, FLAG_CUT if status & (4 | 8) else 0, -1
    if cb + cc > caps[1] or eb + ec > caps[2] or mb + mc > caps[0]:
        return DEAD, FLAG_CUT, -1
    return JOB, 0, f


def np_rough(L, views, trace_min, class_index=-1, caps=None, fill=FILL):
    """The header's comment on exported lists -> (n_live, header flags, states, flags, records ROUGH_POSE_DTYPE, member_group)"""
    caps = caps or (len(L.matches), len(L.clusters), len(L.members))
    n_live = min(int(L.header[3]), caps[1])
    hflags = FLAG_CUT if (int(L.header[1]) & 1) or int(L.header[3]) > caps[1] else 0
    states, flags = [], []
    recs = np.zeros(n_live, ROUGH_POSE_DTYPE)
    group = np.full(caps[2], fill, np.uint32).view(np.int32)
    trace_min = f8(trace_min)
    for k in range(n_live):
        state, fl, f = _frame_of(L, k, caps)
        if state == JOB:
            state, fl = _slot(L, views, trace_min, class_index, caps, k, f, recs, group)
        states.append(state)
        flags.append(fl)
    return n_live, hflags, states, flags, recs, group


def _slot(L, views, trace_min, class_index, caps, k, f, recs, group):
    mbegin, mcount = int(L.frame_info[f, 0]), int(L.frame_info[f, 1])
    c = L.clusters[k]
    b, n = int(c["member_begin"]), int(c["member_count"])
    if n < 1 or b < 0 or b + n > min(int(L.header[4]), caps[2]):
        return BROKEN, FLAG_BOUNDS
    mem = [int(v) for v in L.members[b:b + n]]
    if not 0 <= mem[0] < mcount:
        return BROKEN, FLAG_BOUNDS
    if any(not 0 <= m < mcount for m in mem):
        return BROKEN, FLAG_BOUNDS
    ms = [L.matches[mbegin + m] for m in mem]
    first_class = int(ms[0]["class_index"])
    if any(int(m["class_index"]) != first_class for m in ms):
        return BROKEN, FLAG_BOUNDS
    if class_index >= 0 and first_class != class_index:
        return NO_JOB_CLASS, 0
    if any(not 0 <= int(m["template_id"]) < len(views) for m in ms):
        return NO_JOB_BOUNDS, FLAG_BOUNDS
    tids = [int(m["template_id"]) for m in ms]
    fronts = np.zeros((0, 9))
    sizes, front_match = [], []
    rec = recs[k]
    for p, t in enumerate(tids):
        same = trace_dot(views.R[t], fronts) > trace_min
        if same.any():
            g = int(np.argmax(same))
        else:
            if len(sizes) == MAX_GROUPS:
                group[b + p:b + n] = -1
                rec["n_members"], rec["n_groups"], rec["status"] = n, MAX_GROUPS, TOO_MANY_GROUPS
                return JOB, 0
            g = len(sizes)
            fronts = np.concatenate([fronts, views.R[t:t + 1]])
            sizes.append(0)
            front_match.append(mbegin + mem[p])
        sizes[g] += 1
        group[b + p] = g
    win = winning_group(sizes)
    q = [f8(0)] * 4
    dist = D = ori = f8(0)
    sx = sy = count = hole = 0
    for p, t in enumerate(tids):
        if group[b + p] != win:
            continue
        for j in range(4):
            q[j] = q[j] + views.q[t, j]
        dist, D, ori = dist + views.distance[t], D + views.D[t], ori + views.ori_dist[t]
        sx, sy, count = sx + int(ms[p]["x"]), sy + int(ms[p]["y"]), count + 1
        if abs(views.D[t] - views.ori_dist[t]) < f8(0.001):
            hole = 1
    mx, my = (abs(sx) // count) * (1 if sx >= 0 else -1), (abs(sy) // count) * (1 if sy >= 0 else -1)     # C++'s truncating division
    if abs(mx) > MAX_MEAN or abs(my) > MAX_MEAN:
        return NO_JOB_BOUNDS, FLAG_BOUNDS
    dn = f8(count)
    rec["distance"], rec["D"], rec["ori_dist"], rec["x"], rec["y"] = dist / dn, D / dn, ori / dn, mx, my
    rec["n_members"], rec["n_groups"], rec["group"], rec["n_group_members"], rec["front"], rec["center_hole"] = n, len(sizes), win, count, front_match[win], hole
    x, y, z, w = (v / dn for v in q)
    n2 = ((x * x + y * y) + z * z) + w * w
    if not n2 > 0 or not np.isfinite(n2):
        rec["status"] = DEGENERATE
        return JOB, 0
    ln = np.sqrt(n2)
    rec["R"] = rot_of_quat(x / ln, y / ln, z / ln, w / ln)
    rec["status"] = OK
    return JOB, 0


# ---- the CPU build of the header --------------------------------------------------------------------------------------------------------------

def build_host(directory, sanitize=False):
    exe = os.path.join(str(directory), "rough_pose_host" + ("_san" if sanitize else ""))
    subprocess.check_call(["g++"] + prc.HOST_FLAGS + (pcc.SANITIZE if sanitize else []) + [HOST_SRC, "-o", exe])
    return exe


def run_host(exe, directory, L, views, trace_min, class_index=-1, caps=None, fill=FILL):
    """The CPU build on the lists cut to `caps` -> what np_rough returns, plus the quaternions it computed"""
    caps = caps or (len(L.matches), len(L.clusters), len(L.members))
    head = np.asarray([len(L.frame_info), caps[0], caps[1], caps[2], len(views), class_index, 0, 0], np.int32)
    head[6:7] = np.asarray([fill], np.uint32).view(np.int32)
    ints = [head, L.header.view(np.int32), L.frame_info.reshape(-1), np.ascontiguousarray(L.matches[:caps[0]]).view(np.int32).reshape(-1),
            np.ascontiguousarray(L.clusters[:caps[1]]).view(np.int32).reshape(-1), L.members[:caps[2]]]
    table = np.concatenate([views.R, views.distance[:, None]], 1)
    doubles = [np.asarray([trace_min], f8), table.reshape(-1), views.D, views.ori_dist]
    src, dst = os.path.join(str(directory), "rough_in.bin"), os.path.join(str(directory), "rough_out.bin")
    with open(src, "wb") as fh:
        fh.write(b"".join(np.ascontiguousarray(p, np.int32).tobytes() for p in ints) + b"".join(np.ascontiguousarray(p, f8).tobytes() for p in doubles))
    res = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    raw = open(dst, "rb").read()
    n_live, hflags = (int(v) for v in np.frombuffer(raw, np.int32, 2))
    slot = np.dtype([("state", "<i4"), ("flags", "<i4"), ("rec", ROUGH_POSE_DTYPE)])
    slots = np.frombuffer(raw, slot, n_live, 8)
    at = 8 + n_live * slot.itemsize
    group = np.frombuffer(raw, np.int32, caps[2], at)
    q = np.frombuffer(raw, f8, len(views) * 4, at + caps[2] * 4).reshape(-1, 4)
    assert at + caps[2] * 4 + q.nbytes == len(raw)
    return n_live, hflags, slots["state"].tolist(), slots["flags"].tolist(), slots["rec"].copy(), group.copy(), q


# ---- rotations and lists --------------------------------------------------------------------------------------------------------------------

def rot(axis, deg):
    a = np.deg2rad(f8(deg))
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)]["xyz".index(axis)]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def trace_min_of(deg):
    """lmx_rough_trace_min, restated"""
    return f8(1) + f8(2) * np.cos(f8(deg) * f8(np.pi) / f8(180))


def members_lists(tids, xy=None, cls=0, extra_front=True, tail_frame=False):
    """One frame with one cluster per entry of `tids` (a list of template ids, in member order), behind a first frame that makes every
    begin non-zero.  The matches of a cluster are its members in order; xy: per cluster a list of (x, y), default (40 + p, 30 - p)."""
    rows, clusters = [], []
    for k, ids in enumerate(tids):
        first = len(rows)
        for p, t in enumerate(ids):
            x, y = xy[k][p] if xy is not None and xy[k] is not None else (40 + p % 7, 30 - p % 5)
            rows.append((x, y, 70.0 + (p % 13), t, cls))
        clusters.append(list(range(first, first + len(ids))))
    frames = [(0, pcc.matches_of(rows), clusters)]
    if extra_front:
        frames.insert(0, (0, pcc.matches_of([(5, 6, 60.0, 0, cls), (7, 8, 61.0, 0, cls)]), [[1, 0]]))
    if tail_frame:                                                                        # a second frame without clusters
        frames.append((0, pcc.matches_of([(1, 1, 50.0, 0, cls)]), []))
    return pcc.build_lists(frames)


# ---- meshes for the render --------------------------------------------------------------------------------------------------------------------

def box_mesh(sx=0.06, sy=0.04, sz=0.03):
    """12 triangles"""
    v = np.asarray([[x, y, z] for x in (-sx / 2, sx / 2) for y in (-sy / 2, sy / 2) for z in (-sz / 2, sz / 2)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = []
    for a, b, c, d in quads:
        tri += [[v[a], v[b], v[c]], [v[a], v[c], v[d]]]
    return np.ascontiguousarray(tri, f8)


def tetrahedron(s=0.05):
    v = np.asarray([[s, s, s], [s, -s, -s], [-s, s, -s], [-s, -s, s]], f8) * 0.5
    return np.ascontiguousarray([[v[0], v[1], v[2]], [v[0], v[3], v[1]], [v[0], v[2], v[3]], [v[1], v[3], v[2]]], f8)


# ---- the cases: each rule of the header on lists built for it ------------------------------------------------------------------------------
class Case:
    """expect(states, flags, recs, group, L): asserts what the case was built for, on the CPU build's output"""

    def __init__(self, name, L, views, trace_min, expect, class_index=-1, caps=None):
        self.name, self.L, self.views, self.trace_min, self.expect, self.class_index, self.caps = name, L, views, f8(trace_min), expect, class_index, caps


Z_STEPS = None


def z_steps():
    """513 views: rotations about z in 0.5 degree steps; with a threshold of 0.25 degrees every view is a group of its own"""
    global Z_STEPS
    if Z_STEPS is None:
        Z_STEPS = Views([rot("z", 0.5 * k) for k in range(513)], 0.5)
    return Z_STEPS


def groups_of(L, group, k):
    c = L.clusters[k]
    return group[c["member_begin"]:c["member_begin"] + c["member_count"]].tolist()


def sized_members(sizes):
    """Members so that group g (view g, created g-th) ends with sizes[g] members: one of each in order, then the rest round robin"""
    ids = list(range(len(sizes)))
    left = [s - 1 for s in sizes]
    while any(left):
        for g, n in enumerate(left):
            if n:
                ids.append(g)
                left[g] -= 1
    return ids


# a rotation whose quaternion (.5, -.5, .5, .5) is exact, and the same with a diagonal entry of -1e-300 (the trace stays non-positive) that
# sends quat_of through the branch i = 1: the quaternion comes out as its exact negative
Q_PLUS = np.asarray([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
Q_MINUS = Q_PLUS.copy()
Q_MINUS[0, 0] = -1e-300


def cases():
    out = []
    th10 = trace_min_of(10.0)

    # 1  first fit depends on the order
    abc = Views([rot("z", 0.0), rot("z", 6.0), rot("z", 12.0)], [0.5, 0.55, 0.6])

    def order(states, flags, recs, group, L):
        assert states[1:] == [JOB] * 3 and recs["status"][1:].tolist() == [OK] * 3
        assert [groups_of(L, group, k) for k in (1, 2, 3)] == [[0, 0, 1], [0, 0, 0], [0, 0, 1]]
        assert recs["n_groups"][1:].tolist() == [2, 1, 2] and recs["n_group_members"][1:].tolist() == [2, 3, 2]
        mb = int(L.frame_info[1, 0])
        assert recs["front"][1:].tolist() == [mb + 0, mb + 3, mb + 6]                      # A, B and C opened the winners
    out.append(Case("first_fit_order", members_lists([[0, 1, 2], [1, 0, 2], [2, 1, 0]]), abc, th10, order))

    # 2  the strict boundary
    pq = Views([rot("x", 20.0) @ rot("z", 3.0), rot("x", 20.0) @ rot("y", 4.0)], 0.5)
    tr = trace_dot(pq.R[1], pq.R[:1])[0]
    def grouped_as(want):
        def check(states, flags, recs, group, L):
            assert groups_of(L, group, 1) == want and recs["n_groups"][1] == len(set(want))
        return check
    out.append(Case("boundary_at_tr", members_lists([[0, 1]]), pq, tr, grouped_as([0, 1])))                                  # tr > tr is false: not the same
    out.append(Case("boundary_one_ulp_below", members_lists([[0, 1]]), pq, np.nextafter(tr, -np.inf), grouped_as([0, 0])))

    # 3  ties of size
    zs, th_z = z_steps(), trace_min_of(0.25)
    rng = np.random.RandomState(11)
    for name, sizes in (("two_equal", [2, 2]), ("three_equal_behind_one", [1, 3, 3, 3]), ("ties_17", rng.randint(1, 4, 17).tolist()),
                        ("ties_40", rng.randint(1, 4, 40).tolist()), ("ties_200", rng.randint(1, 3, 200).tolist())):
        def ties(states, flags, recs, group, L, sizes=sizes):
            assert recs["status"][1] == OK and recs["n_groups"][1] == len(sizes)
            assert np.bincount(groups_of(L, group, 1)).tolist() == sizes
            assert sizes[recs["group"][1]] == max(sizes) == recs["n_group_members"][1]
            if len(sizes) <= 16:
                assert recs["group"][1] == sizes.index(max(sizes))                           # the earliest
        out.append(Case(name, members_lists([sized_members(sizes)]), zs, th_z, ties))

    # 4  every branch of the matrix-to-quaternion
    n = np.asarray([0.1, 0.5, 0.85])
    n = n / np.linalg.norm(n)
    branch = Views([rot("z", 30.0), rot("x", 180.0), rot("y", 180.0), rot("z", 180.0), 2.0 * np.outer(n, n) - np.eye(3)], 0.5)
    assert branch.R[4, 4] > branch.R[4, 0] and branch.R[4, 8] > branch.R[4, 4]

    def branches(states, flags, recs, group, L):
        assert recs["status"][1:].tolist() == [OK] * 5
        for k in range(5):
            assert np.abs(recs["R"][1 + k] - branch.R[k]).max() < 1e-12, k                  # one member: the mean is the view
    out.append(Case("quaternion_branches", members_lists([[k] for k in range(5)]), branch, th10, branches))

    # 5  sign: no alignment
    sign = Views([Q_PLUS, Q_MINUS, rot("x", 40.0), rot("z", 179.0), rot("z", -179.0)], 0.5)
    assert sign.q[0].tolist() == [0.5, -0.5, 0.5, 0.5] and sign.q[1].tolist() == [-0.5, 0.5, -0.5, -0.5]
    assert sign.q[3, 3] > 0 > sign.q[4, 3] and sign.q[3, 2] > 0 and sign.q[4, 2] > 0

    def signs(states, flags, recs, group, L):
        assert recs["status"][1:].tolist() == [OK, DEGENERATE, OK] and recs["n_groups"][1:].tolist() == [1, 1, 1]
        assert np.abs(recs["R"][1] - sign.R[2]).max() < 1e-12                               # +q - q + q3: the sum's, not (2 q + q3)'s
        assert not recs["R"][2].any() and recs["n_group_members"][2] == 2 and recs["distance"][2] == 0.5
        assert np.abs(recs["R"][3] - rot("z", 180.0).reshape(9)).max() < 1e-12              # w cancels, z adds: half a turn
    out.append(Case("sign", members_lists([[0, 1, 2], [0, 1], [3, 4]]), sign, -3.0, signs))

    # 6  counts
    three = Views([rot("y", 0.0), rot("y", 4.0), rot("y", 30.0), rot("y", 34.0), rot("y", 70.0)], [0.4, 0.45, 0.5, 0.55, 0.6])
    ids65 = [(p * 7) % 5 for p in range(65)]
    ids130 = [(p * 3) % 5 for p in range(130)]

    def counts(states, flags, recs, group, L):
        assert recs["status"][1:].tolist() == [OK] * 3 and recs["n_members"][1:].tolist() == [1, 65, 130] and recs["n_groups"][1:].tolist() == [1, 3, 3]
    out.append(Case("members_1_65_130", members_lists([[2], ids65, ids130]), three, th10, counts))
    for n_groups, status in ((70, OK), (512, OK), (513, TOO_MANY_GROUPS)):
        ids = list(range(n_groups)) + [n_groups - 1, 5, 5]

        def many(states, flags, recs, group, L, n_groups=n_groups, status=status):
            assert states[1] == JOB and recs["status"][1] == status and recs["n_members"][1] == n_groups + 3
            if status == OK:
                assert recs["n_groups"][1] == n_groups and recs["group"][1] == 5 and recs["n_group_members"][1] == 3
                assert groups_of(L, group, 1) == list(range(n_groups)) + [n_groups - 1, 5, 5]
            else:
                assert recs["n_groups"][1] == MAX_GROUPS and groups_of(L, group, 1) == list(range(512)) + [-1] * 4 and not recs["R"][1].any()
        out.append(Case("groups_%d" % n_groups, members_lists([ids]), zs, th_z, many))

    # 7  truncating means, center_hole
    hole = Views([rot("z", 0.0)] * 3, 0.5, D=[0.000999, 0.001, 0.7], ori_dist=[0.0, 0.0, 0.2])

    def means(states, flags, recs, group, L):
        assert recs["x"][1:].tolist() == [3, -3, 3, 3] and recs["y"][1:].tolist() == [-3, 3, 3, 3]
        assert recs["center_hole"][1:].tolist() == [1, 0, 0, 1]
    out.append(Case("truncating_means", members_lists([[0, 0], [1, 1], [2, 1], [2, 0]], xy=[[(3, -4), (4, -3)], [(-3, 4), (-4, 3)], [(3, 4), (4, 3)], [(3, 4), (4, 3)]]),
                    hole, th10, means))
    out.extend(hostile_cases(abc, th10))
    return out


def hostile_cases(views, tm):
    """Lists no export writes: each gives the state and flag the header states, the slots around it untouched"""
    out = []

    def base():
        m0 = pcc.matches_of([(10 + i, 20 - i, 70.0 + i, i % 3, 0) for i in range(9)])
        m1 = pcc.matches_of([(30 + i, 40 - i, 80.0 + i, (i + 1) % 3, 0) for i in range(8)])
        return pcc.build_lists([(0, m0, [[0, 1], [2, 3, 4], [5, 6, 7, 8]]), (0, m1, [[7], [0, 1, 2], [3, 4, 5, 6]])])

    def expect_at(k, state, flag):
        def check(states, flags, recs, group, L):
            assert (states[k], flags[k]) == (state, flag), (states, flags)
            assert not recs[k:k + 1].view(np.uint8).any()
            assert all(s == JOB and f == 0 for i, (s, f) in enumerate(zip(states, flags)) if i != k)
            c = L.clusters[k]
            if state != JOB and 0 <= c["member_begin"] and c["member_begin"] + max(int(c["member_count"]), 0) <= len(group):
                assert (group[c["member_begin"]:c["member_begin"] + c["member_count"]].view(np.uint32) == FILL).all()
        return check

    def add(name, change, k, state, flag, **kw):
        L = base()
        change(L)
        out.append(Case("hostile_" + name, L, views, tm, expect_at(k, state, flag), **kw))

    def member(i, v):
        return lambda L: L.members.__setitem__(i, v)

    def match(i, field, v):
        return lambda L: L.matches[field].__setitem__(i, v)

    def cluster(k, field, v):
        return lambda L: L.clusters[field].__setitem__(k, v)
    add("member_minus_one", member(3, -1), 1, BROKEN, FLAG_BOUNDS)
    add("member_at_match_count", member(4, 9), 1, BROKEN, FLAG_BOUNDS)
    add("first_member_far", member(2, -(1 << 31)), 1, BROKEN, FLAG_BOUNDS)
    add("template_minus_one", match(3, "template_id", -1), 1, NO_JOB_BOUNDS, FLAG_BOUNDS)
    add("template_at_n_views", match(4, "template_id", 3), 1, NO_JOB_BOUNDS, FLAG_BOUNDS)
    add("template_far", match(2, "template_id", (1 << 31) - 1), 1, NO_JOB_BOUNDS, FLAG_BOUNDS)
    add("class_mix", match(4, "class_index", 1), 1, BROKEN, FLAG_BOUNDS, class_index=0)
    add("class_mix_every_class", match(3, "class_index", 1), 1, BROKEN, FLAG_BOUNDS)

    def other_class(L):
        L.matches["class_index"][2:5] = 1
        L.matches["template_id"][3] = 77                                                  # another class's table: not looked at
    add("first_member_other_class", other_class, 1, NO_JOB_CLASS, 0, class_index=0)
    add("member_count_zero", cluster(1, "member_count", 0), 1, BROKEN, FLAG_BOUNDS)
    add("member_count_huge", cluster(1, "member_count", 1 << 30), 1, BROKEN, FLAG_BOUNDS)
    add("member_begin_negative", cluster(1, "member_begin", -1), 1, BROKEN, FLAG_BOUNDS)

    def mean_far(L):
        L.matches["x"][2:5] = (1 << 17) + 1
    L = base()
    L.matches["x"][2:5] = (1 << 17) + 1

    def mean_far(states, flags, recs, group, L):                                          # decided behind the groups: member_group is written
        assert (states[1], flags[1]) == (NO_JOB_BOUNDS, FLAG_BOUNDS) and not recs[1:2].view(np.uint8).any() and groups_of(L, group, 1) == [0, 1, 0]
    out.append(Case("hostile_mean_beyond_2_17", L, views, tm, mean_far))

    # a member range beyond cap_members: the frame is cut (dead), as in the pose chain
    L = base()

    def cut(states, flags, recs, group, L):
        assert states == [JOB, JOB, JOB, DEAD, DEAD, DEAD] and flags[3:] == [FLAG_CUT] * 3 and not recs[3:].view(np.uint8).any()
    out.append(Case("hostile_members_beyond_cap", L, views, tm, cut, caps=(len(L.matches), len(L.clusters), len(L.members) - 1)))

    # overlapping frames
    L = base()
    L.frame_info[1, 2] = 1

    def overlap(states, flags, recs, group, L):
        assert states == [JOB, BROKEN, BROKEN, JOB, DEAD, DEAD] and flags == [0, FLAG_BOUNDS, FLAG_BOUNDS, 0, 0, 0]
    out.append(Case("hostile_overlapping_frames", L, views, tm, overlap))
    return out
