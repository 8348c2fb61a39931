"""Tap tuples for the depth quantiser's stage before the median (np_restatement.normal_bin_of_taps), and images that carry them.

A pixel of quantizedNormals sees the image through nine values: its depth d and the eight neighbours at distance 5.  With all of
them valid the normal is proportional to (115 B0, 115 B1, -3 d) (B0, B1 the delta sums); in general to (230 X, 230 Y, -D d) with
X = a3 B0 - a1 B1, Y = a0 B1 - a1 B0, D = a0 a3 - a1^2 over the tap counts a0, a3, a1.  The label changes where 10 nx/|n| or 20 nz/|n|
crosses an integer, and only a tuple that sits within a float32 rounding error of such a crossing can tell a correctly rounded
sqrt / divide from one that is an ulp off.  Three families, all deterministic:

  S  ulp-sensitive tuples (moving s or inv by one float32 ulp changes the flat index) and exact lattice points, found by the search
     below and kept in tests/golden/depth_normal_sensitive.npz (tests/golden/make_depth_normal_sensitive.py);
  V  validity and range edges: every mask, deltas around +-thr, thr <= 0, d at 0 / distance_threshold / 65535, the largest operands
     the 24-bit products of the int32 form ever see;
  R  a million random tuples.

block_image() lays tuples out as an image: constant 5x5 blocks, a case every third block, so that all 25 pixels of a case's centre
block have exactly the case's taps and the 5x5 median at the block's centre is unanimous.
"""
import functools
import os

import numpy as np

import np_restatement as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_normal_sensitive.npz")
INT_THRESHOLDS = (50, 200)        # the int32 form (difference_threshold <= 200)
LONG_THRESHOLDS = (201, 5000)     # the 64-bit form
FAR = 70000                       # a distance_threshold no u16 depth reaches


# ---- sensitivity ----------------------------------------------------------------------------------------------
def sensitive(taps, dist, thr):
    """True where replacing s by either float32 neighbour, or inv by either neighbour, changes the flat index."""
    idx = R.normal_bin_of_taps(taps, dist, thr)[1]
    out = np.zeros(len(idx), bool)
    for kw in (dict(s_ulps=1), dict(s_ulps=-1), dict(inv_ulps=1), dict(inv_ulps=-1)):
        out |= R.normal_bin_of_taps(taps, dist, thr, **kw)[1] != idx
    return out


def _reduced(taps, thr):
    """(230 X, 230 Y, D d) in int64: the normal divided by 625, exact."""
    t = np.asarray(taps).astype(np.int64)
    d = t[:, 0]
    thr = np.broadcast_to(np.asarray(thr, np.int64), d.shape)
    delta = t[:, 1:] - d[:, None]
    f = (np.abs(delta) < thr[:, None]).astype(np.int64)
    md = f * delta
    a0 = f[:, 0] + f[:, 2] + f[:, 3] + f[:, 4] + f[:, 5] + f[:, 7]
    a3 = f[:, 0] + f[:, 1] + f[:, 2] + f[:, 5] + f[:, 6] + f[:, 7]
    a1 = f[:, 0] + f[:, 7] - f[:, 2] - f[:, 5]
    B0 = (md[:, 2] + md[:, 4] + md[:, 7]) - (md[:, 0] + md[:, 3] + md[:, 5])
    B1 = (md[:, 5] + md[:, 6] + md[:, 7]) - (md[:, 0] + md[:, 1] + md[:, 2])
    return 230 * (a3 * B0 - a1 * B1), 230 * (a0 * B1 - a1 * B0), (a0 * a3 - a1 * a1) * d


def lattice(taps, dist, thr):
    """True where the exact real 10 nx/|n|, 10 ny/|n| or 20 nz/|n| is an integer and the normal is not along z (integer test)."""
    X, Y, Z = _reduced(taps, thr)
    n2 = X * X + Y * Y + Z * Z
    assert n2.max(initial=0) < 1 << 54   # 400 k^2 n2 stays inside int64
    out = np.zeros(len(X), bool)
    safe = np.maximum(n2, 1).astype(np.float64)
    for c, scale in ((X, 10), (Y, 10), (Z, 20)):
        k = np.rint(np.sqrt(scale * scale * (c * c).astype(np.float64) / safe)).astype(np.int64)
        out |= (scale * scale * c * c == k * k * n2) & (c != 0)
    tilted = (X != 0) | (Y != 0)
    return out & tilted & (n2 > 0) & (np.asarray(taps)[:, 0] < dist)


def _near_boundary(taps, dist, thr, tol=3e-5):
    """Cheap float64 filter in front of sensitive(): a component within tol of an integer (a float32 ulp at 20 is 1.9e-6)."""
    X, Y, Z = _reduced(taps, thr)
    n = np.sqrt((X * X + Y * Y + Z * Z).astype(np.float64))
    ok = (n > 0) & (np.asarray(taps)[:, 0] < dist)
    n = np.where(ok, n, 1.0)
    near = np.zeros(len(X), bool)
    for c, scale in ((X, 10.0), (Y, 10.0), (Z, 20.0)):
        u = scale * c / n
        near |= np.abs(u - np.rint(u)) < tol
    return near & ok


# ---- the search -------------------------------------------------------------------------------------------------
# A slice is a few hundred thousand to a few million candidate tuples built from a short description; the fixture is what survives
# of all slices, and a test can re-run any one of them.
def _grid_slice(thr, dist, corners, d_values, reach):
    """Mid taps carry B0 = i and B1 = j (both signs), valid corners sit at d, invalid corners at d +- thr; D = 36, 24, 20, 16, 12 ..."""
    r = np.arange(-reach, reach + 1, dtype=np.int64)
    dd, jj, ii = (a.reshape(-1) for a in np.meshgrid(np.asarray(d_values, np.int64), r, r, indexing="ij"))
    t = np.empty((len(dd), 9), np.int64)
    t[:, 0] = dd
    hi_i, hi_j = (ii + 1) // 2, (jj + 1) // 2
    t[:, 5] = dd + hi_i; t[:, 4] = dd + hi_i - ii      # taps 4 (0, +5) and 3 (0, -5): md4 - md3 = i
    t[:, 7] = dd + hi_j; t[:, 2] = dd + hi_j - jj      # taps 6 (+5, 0) and 1 (-5, 0): md6 - md1 = j
    for bit, col in enumerate((1, 3, 6, 8)):            # corner taps 0, 2, 5, 7
        off = 0 if corners >> bit & 1 else thr
        t[:, col] = np.where(dd + off <= 65535, dd + off, dd - off)
    keep = (t.min(1) >= 0) & (t.max(1) <= 65535)
    return t[keep]


def _plane_slice(thr, dist, d_values, reach, step):
    """All nine values on a plane d + x sign(i) + y sign(j): every tap valid, B0 = 3 i and B1 = 3 j -- slopes steep enough to reach a
    boundary at depths up to 65535."""
    r = np.arange(-reach, reach + 1, step, dtype=np.int64)
    dd, jj, ii = (a.reshape(-1) for a in np.meshgrid(np.asarray(d_values, np.int64), r, r, indexing="ij"))
    hi_i, hi_j = (ii + 1) // 2, (jj + 1) // 2
    t = np.empty((len(dd), 9), np.int64)
    t[:, 0] = dd
    for k, (j, i) in enumerate(R.TAP_OFFSETS):
        t[:, 1 + k] = dd + (hi_i if i > 0 else hi_i - ii if i < 0 else 0) + (hi_j if j > 0 else hi_j - jj if j < 0 else 0)
    keep = (t.min(1) >= 0) & (t.max(1) <= 65535) & (np.abs(t[:, 1:] - dd[:, None]).max(1) < thr)
    return t[keep]


def _random_slice(thr, dist, d_max, n, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, d_max + 1, n)
    delta = rng.integers(-thr - 2, thr + 3, (n, 8))
    return np.clip(np.concatenate([d[:, None], d[:, None] + delta], 1), 0, 65535)


def slices():
    out = []
    for thr in INT_THRESHOLDS + LONG_THRESHOLDS:
        reach = 36
        for corners in (15, 14, 9, 6, 5, 0, 7, 3):
            for lo in range(1, 2000, 400):
                out.append(("grid", thr, 2000, corners, (lo, min(lo + 400, 2000), 1), reach))
        for lo in range(2000, 65536, 12800):
            out.append(("plane", thr, FAR, (lo, min(lo + 12800, 65536), 101), min(thr - 1, 96) // 2 * 2, 1 if thr <= 50 else 2))
        for k in range(6):
            out.append(("random", thr, 2000, 1999, 1 << 21, 1000 * thr + k))
        for k in range(3):
            out.append(("random", thr, FAR, 65535, 1 << 21, 1000 * thr + 500 + k))
    return out


def candidates(desc):
    if desc[0] == "grid":
        _, thr, dist, corners, (lo, hi, step), reach = desc
        return _grid_slice(thr, dist, corners, np.arange(lo, hi, step), reach), dist, thr
    if desc[0] == "plane":
        _, thr, dist, (lo, hi, step), reach, stride = desc
        return _plane_slice(thr, dist, np.arange(lo, hi, step), reach, stride), dist, thr
    _, thr, dist, d_max, n, seed = desc
    return _random_slice(thr, dist, d_max, n, seed), dist, thr


def search_slice(desc):
    """-> (taps u16 [m, 9], dist, thr, sensitive [m], lattice [m]) of the slice's rows that are sensitive or lattice points."""
    t, dist, thr = candidates(desc)
    t = t[_near_boundary(t, dist, thr)]
    s, l = sensitive(t, dist, thr), lattice(t, dist, thr)
    keep = s | l
    return t[keep].astype(np.uint16), dist, thr, s[keep], l[keep], len(keep)


@functools.lru_cache(maxsize=None)
def load_fixture():
    """the arrays of tests/golden/depth_normal_sensitive.npz (shared between tests: read only)"""
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


# ---- V: validity and range edges ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_v():
    """-> list of (taps [n, 9] u16, dist, thr).  One entry per (dist, thr) pair."""
    out = []
    for thr in (1, 2, 50, 199, 200, 201, 5000, 70000, 0, -5):
        for dist in (2000, FAR):
            rows = []
            edge = sorted({s * (abs(thr) + o) for s in (-1, 1) for o in (-2, -1, 0, 1)} | {0})
            d_list = [0, 1, dist - 1, dist, 65535, 1000, 30000] if dist <= 65535 else [0, 1, 65535, 1000, 30000, 65535 - abs(thr), abs(thr)]
            for d in d_list:
                if not 0 <= d <= 65535:
                    continue
                # every mask: an invalid tap sits at distance thr, a valid one at the largest valid distance, signs by position
                for mask in range(256):
                    for flip in (1, -1):
                        row = [d]
                        for k in range(8):
                            sgn = flip * (1 if k in (2, 4, 7, 6) else -1)
                            dl = sgn * (abs(thr) - 1 if mask >> k & 1 else abs(thr))
                            row.append(d + dl)
                        rows.append(row)
                # one tap walks over the edge deltas, with 0 and 65535 thrown in, the others stay level or tilt
                for k in range(8):
                    for e in edge:
                        for base in (0, 1, -1):
                            row = [d] + [d + base * (1 if kk in (2, 4, 7) else -1 if kk in (0, 3, 5) else 0) for kk in range(8)]
                            row[1 + k] = d + e
                            rows.append(row)
                    for v in (0, 65535):
                        row = [d] * 9
                        row[1 + k] = v
                        rows.append(row)
                rows.append([d] + [0] * 8)
                rows.append([d] + [65535] * 8)
                rows.append([d] * 9)                                     # det > 0, ddx = ddy = 0
                rows.append([d, 60000, d, 60000, 60000, 60000, 60000, d, 60000] if abs(d - 60000) >= abs(thr) else [d] * 9)
            if thr > 1:
                # the largest operands: every right (lower) tap at +(thr-1), every left (upper) tap at -(thr-1), d as large as it goes
                # (a u16 image cannot have both at d = 65535: there the slope is one-sided)
                m = thr - 1
                for d in (65535 - m, 65535, m, 0, 30000):
                    for sx, sy in ((1, 0), (0, 1), (1, 1), (1, -1), (-1, 0), (0, -1), (-1, -1), (-1, 1)):
                        c = [int(np.clip(sx * np.sign(i) + sy * np.sign(j), -1, 1)) for j, i in R.TAP_OFFSETS]
                        rows.append([d] + [d + m * v for v in c])
                        rows.append([d] + [d + m * min(v, 0) for v in c])
                        rows.append([d] + [d + m * max(v, 0) for v in c])
            # valid taps on one line through the pixel: det == 0, and then ddx = ddy = 0 too (ss == 0)
            if thr > 2:
                for d in (1, 500, 65535 - abs(thr)):
                    far_tap = d + thr if d + thr <= 65535 else d - thr
                    for pair, dl in (((3, 4), (-1, 1)), ((1, 6), (-1, 1)), ((3,), (2,)), ((0, 7), (-1, 1)), ((2, 5), (1, -1))):
                        row = [d] + [far_tap] * 8
                        for k, v in zip(pair, dl):
                            row[1 + k] = d + v
                        rows.append(row)
            t = np.asarray(rows, np.int64)
            t = t[(t.min(1) >= 0) & (t.max(1) <= 65535)]
            out.append((np.unique(t, axis=0).astype(np.uint16), dist, thr))
    return out


# ---- R: random ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_r():
    """-> list of (taps, dist, thr); 1.25 million tuples in all."""
    out = []
    for k, (thr, dist, d_max, n) in enumerate(((50, 2000, 2050, 300000), (200, 2000, 2050, 300000), (201, 2000, 2050, 150000),
                                               (5000, 2000, 2050, 150000), (50, FAR, 65535, 100000), (200, FAR, 65535, 100000),
                                               (199, 30000, 30050, 50000), (5000, FAR, 65535, 100000))):
        out.append((_random_slice(thr, dist, d_max, n, 7000 + k).astype(np.uint16), dist, thr))
    return out


# ---- block images -----------------------------------------------------------------------------------------------------
def block_capacity(H, W):
    """cases a block image of this size holds: a case takes 15 x 15 pixels and its centre block must lie inside the r = 5 frame
    (rows 5 .. H - 7), which the layout gives as long as 15 rows + 1 <= H."""
    return ((H - 1) // 15), ((W - 1) // 15)


def block_centres(n, H, W):
    """centre pixel (y, x) of the first n cases of a block image, row-major."""
    rows, cols = block_capacity(H, W)
    assert n <= rows * cols, (n, rows, cols)
    k = np.arange(n)
    return 15 * (k // cols) + 7, 15 * (k % cols) + 7


def block_image(taps, H, W, fill=0):
    """u16 image H x W, constant on 5x5 blocks: case k's depth fills block (3 r + 1, 3 c + 1) and its eight taps the blocks around it,
    so every pixel of the centre block has exactly the case's taps.  What the cases do not cover is `fill`."""
    taps = np.asarray(taps, np.uint16).reshape(-1, 9)
    rows, cols = block_capacity(H, W)
    assert len(taps) <= rows * cols, (len(taps), rows, cols)
    blocks = np.full((3 * rows, 3 * cols), fill, np.uint16)
    k = np.arange(len(taps))
    by, bx = 3 * (k // cols) + 1, 3 * (k % cols) + 1
    blocks[by, bx] = taps[:, 0]
    for c, (j, i) in enumerate(R.TAP_OFFSETS):
        blocks[by + j // 5, bx + i // 5] = taps[:, 1 + c]
    img = np.full((H, W), fill, np.uint16)
    img[:15 * rows, :15 * cols] = np.kron(blocks, np.ones((5, 5), np.uint16))
    return img


def taps_of_image(depth):
    """-> (taps [n, 9], ys, xs) of every pixel inside the r = 5 frame (rows 5 .. H - 7, columns 5 .. W - 7), row-major."""
    d = np.asarray(depth)
    H, W = d.shape
    ys, xs = np.mgrid[5:H - 6, 5:W - 6]
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    return np.stack([d[ys, xs]] + [d[ys + j, xs + i] for j, i in R.TAP_OFFSETS], 1), ys, xs


def quantized_from_taps(depth, dist, thr, **mutant):
    """quantizedNormals of an image through the per-tuple restatement -> (after the median, before the median)."""
    t, ys, xs = taps_of_image(depth)
    pre = np.zeros(np.asarray(depth).shape, np.uint8)
    pre[ys, xs] = R.bin_to_label(R.normal_bin_of_taps(t, dist, thr, **mutant)[0])
    return R.median5(pre), pre


# ---- the device hook ----------------------------------------------------------------------------------------------------
def digit_tables():
    """Five NORMAL_LUTs that spell the flat index in base 8: table k gives index i the label 1 << ((i >> 3 k) & 7), so bin - 1 is
    digit k and bin 0 still means `no look-up`."""
    i = np.arange(8000)
    return [(1 << ((i >> (3 * k)) & 7)).astype(np.uint8) for k in range(5)]


def device_bins(taps, dist, thr, variant, lut=None):
    from linemod_pose_estimation_amd import _lib
    t = np.ascontiguousarray(taps, np.uint16).reshape(-1, 9)
    out = np.full(len(t), 0xee, np.uint8)
    table = None if lut is None else np.ascontiguousarray(lut, np.uint8).reshape(8000)
    _lib.check(_lib.lib().lmx_debug_depth_normal_bins(0, t.ctypes.data, len(t), int(dist), int(thr), int(variant),
                                                      None if table is None else table.ctypes.data, out.ctypes.data))
    return out


def device_flat_index(taps, dist, thr, variant):
    """the flat index of the device's look-up (-1 where it made none), recovered from the bins under the five digit tables."""
    digits = [device_bins(taps, dist, thr, variant, tab).astype(np.int64) for tab in digit_tables()]
    none = digits[0] == 0
    for dg in digits:
        assert np.array_equal(dg == 0, none) and dg.max(initial=0) <= 8    # a look-up happens under every table or under none
    return np.where(none, -1, sum((dg - 1) << (3 * k) for k, dg in enumerate(digits)))
