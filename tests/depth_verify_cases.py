"""The depth check of matches (lmx_depth_diff_matches): its numpy restatement and the constructed crops, scene and match positions shared by
tests/test_depth_verify_host.py (CPU build of csrc/lmx_depth_verify.hpp) and tests/test_gpu_depth_verify.py (the kernel).

Definition: crop t[h][w], scene s[H][W], both uint16 mm, match at (x, y): crop pixel (i, j) meets scene pixel (x + j, y + i) and counts
iff t != 0, the scene pixel lies inside the image and s != 0.  n_template = #(t != 0), n_valid = #counting, sum_abs_mm = sum |t - s|."""
import functools

import numpy as np

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
SCENE_W, SCENE_H = 96, 64
WIDTHS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 129)
HEIGHTS = (1, 3, 4, 5, 9)


def np_diff(crop, scene, x, y):
    """-> (sum_abs_mm, n_valid, n_template) as Python ints; x, y any Python ints (no fixed-width arithmetic here)."""
    h, w = crop.shape
    H, W = scene.shape
    x, y = int(x), int(y)
    n_template = int(np.count_nonzero(crop))
    j0, j1, i0, i1 = max(0, -x), min(w, W - x), max(0, -y), min(h, H - y)
    if j0 >= j1 or i0 >= i1:
        return 0, 0, n_template
    t = crop[i0:i1, j0:j1].astype(np.int64)
    s = scene[y + i0:y + i1, x + j0:x + j1].astype(np.int64)
    ok = (t != 0) & (s != 0)
    return int(np.abs(t - s)[ok].sum()), int(ok.sum()), n_template


def np_diff_matches(crops, frames, matches, offsets, class_index=-1):
    """The batch form -> int64 [n, 3] (sum_abs_mm, n_valid, n_template), zeros for matches of other classes."""
    out = np.zeros((len(matches), 3), np.int64)
    for f in range(len(frames)):
        for i in range(int(offsets[f]), int(offsets[f + 1])):
            m = matches[i]
            if class_index >= 0 and int(m["class_index"]) != class_index:
                continue
            out[i] = np_diff(crops[int(m["template_id"])], frames[f], int(m["x"]), int(m["y"]))
    return out


def _values(rng, shape, zero_share):
    """uint16 values: `zero_share` zeros, a tenth each of 1 and 65535, the rest anything non-zero."""
    v = rng.integers(1, 65536, shape).astype(np.uint16)
    k = rng.random(shape)
    v[k < 0.1] = 1
    v[(k >= 0.1) & (k < 0.2)] = 65535
    v[rng.random(shape) < zero_share] = 0
    return v


def positions(w, h, W=SCENE_W, H=SCENE_H):
    """Match positions for a w x h crop: inside at even and odd x (where the crop fits), cut by each border, negative x / y, entirely
    outside on every side, and the ends of the int32 range."""
    pos = [(10, 7), (11, 7), (0, 0), (W - w, H - h),                 # inside (or, for crops wider than the scene, cut on both sides)
           (-1, 5), (-(w // 2) - 1, 5), (W - (w + 1) // 2, 5), (W - w + 1, 5), (W - 1, 5),     # left / right border
           (10, -1), (10, -(h // 2) - 1), (10, H - (h + 1) // 2), (10, H - h + 1), (10, H - 1),  # top / bottom border
           (-1, -1), (W - 1, H - 1), (-(w // 2) - 1, H - 1),         # corners
           (W, 5), (-w, 5), (10, H), (10, -h), (W + 1000, H + 1000), (-5000, -5000),   # entirely outside
           (INT32_MAX - 1, 5), (INT32_MAX, INT32_MAX), (INT32_MIN, 5), (10, INT32_MIN), (10, INT32_MAX - 1), (INT32_MAX - w, INT32_MAX - h)]
    return pos


@functools.lru_cache(maxsize=None)
def constructed():
    """-> (crops: list of uint16 [h, w], scene uint16 [64, 96], matches: int64 [n, 3] rows (x, y, crop), expected int64 [n, 3]).  Built
    once per session; treat as read-only."""
    rng = np.random.default_rng(20240607)
    scene = _values(rng, (SCENE_H, SCENE_W), 0.2)
    crops = [_values(rng, (h, w), 0.3) for w in WIDTHS for h in HEIGHTS]
    rows = [(x, y, k) for k, c in enumerate(crops) for (x, y) in positions(c.shape[1], c.shape[0])]
    matches = np.asarray(rows, np.int64)
    expected = np.asarray([np_diff(crops[k], scene, x, y) for x, y, k in rows], np.int64)
    # what the list claims to hold
    zs, zc = np.mean(scene == 0), np.mean(np.concatenate([c.ravel() for c in crops]) == 0)
    assert 0.15 < zs < 0.25 and 0.25 < zc < 0.35, (zs, zc)
    assert (expected[:, 1] == 0).sum() > 200 and (expected[:, 1] > 0).sum() > 500
    assert (expected[:, 1] < expected[:, 2]).any() and (matches[:, 0] & 1).any() and not (matches[:, 0] & 1).all()
    lo_hi = hi_lo = False       # crop 1 against scene 65535 and crop 65535 against scene 1 among the counting pixels of inside placements
    for c in crops:
        h, w = c.shape
        if w <= SCENE_W - 11 and h <= SCENE_H - 7:
            s = scene[7:7 + h, 10:10 + w]
            lo_hi = lo_hi or bool(((c == 1) & (s == 65535)).any())
            hi_lo = hi_lo or bool(((c == 65535) & (s == 1)).any())
    assert lo_hi and hi_lo
    return crops, scene, matches, expected


# Crops wider than the 64 vectors (512 pixels) a wave's lanes cover in one trip along a row: 505 has pitch 512, the last single-trip width;
# 513 has 65 vectors, so lane 0 alone takes a second trip; 1100 has 138, two trips for most lanes and three for the first ten.
WIDE_W, WIDE_H = 1200, 12
WIDE_SIZES = ((505, 1), (505, 5), (513, 1), (513, 5), (1100, 5))


def wide_positions(w, h, W=WIDE_W, H=WIDE_H):
    """Inside at an even and at an odd x, cut by the left and by the right border, y = -2, y = H - 3, entirely outside, x = INT32_MAX - w."""
    return [(40, 2), (41, 2), (-(w // 2) - 1, 2), (W - (w + 1) // 2, 2), (40, -2), (40, H - 3), (W, 2), (INT32_MAX - w, 2)]


@functools.lru_cache(maxsize=None)
def wide():
    """-> (crops, scene uint16 [12, 1200], rows int64 [n, 3] (x, y, crop), expected int64 [n, 3]) for the wide crops.  Read-only."""
    rng = np.random.default_rng(20240619)
    crops = [_values(rng, (h, w), 0.3) for w, h in WIDE_SIZES]
    scene = _values(rng, (WIDE_H, WIDE_W), 0.2)
    rows = np.asarray([(x, y, k) for k, c in enumerate(crops) for (x, y) in wide_positions(c.shape[1], c.shape[0])], np.int64)
    expected = np.asarray([np_diff(crops[k], scene, x, y) for x, y, k in rows], np.int64)
    return crops, scene, rows, expected


def match_records(dtype, rows, class_index=0):
    """(x, y, crop) rows -> match records of `dtype` (MATCH_DTYPE)."""
    m = np.zeros(len(rows), dtype)
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    m["x"], m["y"], m["template_id"] = rows[:, 0], rows[:, 1], rows[:, 2]
    m["similarity"], m["class_index"] = 90.0, class_index
    return m
