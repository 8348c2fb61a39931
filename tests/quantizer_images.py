"""Hostile inputs for the two quantisers (colour gradients, depth normals) and the counters that prove the inputs reach the kernels'
decision boundaries.  Test infrastructure only.

synth.make_scene draws tame images: a few depth planes with 0.3 mm noise, a low-frequency colour texture, so a pixel's label is almost
always its neighbours' label, most 5x5 median windows are unanimous and a label written to the wrong place is usually the right label
anyway.  The generators below make every pixel's label its own: depth images whose normals change from pixel to pixel, read through a
random NORMAL_LUT (the label is then a hash of the normal), and colour images whose gradient magnitudes sit at the weak threshold, whose
3x3 votes sit at the 5-of-9 rule and whose channels tie with different orientations.  The counters are plain numpy on top of
np_restatement and the oracle; tests/test_quantizer_images_host.py asserts them on the CPU, tests/test_gpu_quantizer_images.py runs the
same images through every launch path of the device quantisers.
"""
import numpy as np

import np_restatement as R
from oracle import oracle as o

LABEL_VALUES = np.array([0, 1, 2, 4, 8, 16, 32, 64, 128], np.uint8)
CELL = 24                                   # the generators' cell size: no relation to the kernels' 64 x 16 / 64 x 32 tiles
NORMAL_TABLES = {                           # probabilities of the nine label values, in ascending value order
    "uniform": (0.12, 0.11, 0.11, 0.11, 0.11, 0.11, 0.11, 0.11, 0.11),
    "high": (0.04, 0.04, 0.04, 0.04, 0.04, 0.05, 0.10, 0.25, 0.40),
}


def _per_cell(a, H, W):
    return np.kron(a, np.ones((CELL, CELL), a.dtype))[:H, :W]


# ---- depth -----------------------------------------------------------------------------------------------------------------------------
def normal_table(kind, seed=0):
    """A random NORMAL_LUT[20][20][20]: the label becomes a hash of the normal, so neighbouring pixels get independent labels."""
    rng = np.random.default_rng([seed, sorted(NORMAL_TABLES).index(kind)])
    return rng.choice(LABEL_VALUES, (20, 20, 20), p=NORMAL_TABLES[kind])


def hostile_depth(H, W, seed, dist=2000):
    """u16 depth: per 24 x 24 cell a base depth in 300..1899 and a noise amplitude, pixel = base + rint(U(-1, 1) * amplitude); then 4 % holes
    (0), 1 % saturated pixels (65535) and 2 % pixels at the distance threshold (dist - 1, dist, dist + 1)."""
    rng = np.random.default_rng([seed, H, W])
    ch, cw = -(-H // CELL), -(-W // CELL)
    base = rng.integers(300, 1900, (ch, cw))
    amp = rng.choice(np.array([2, 5, 9, 14, 22, 35, 48]), (ch, cw))
    d = _per_cell(base, H, W) + np.rint(rng.uniform(-1.0, 1.0, (H, W)) * _per_cell(amp, H, W)).astype(np.int64)
    u = rng.uniform(0.0, 1.0, (H, W))
    edge = dist - 1 + rng.integers(0, 3, (H, W))
    d = np.where(u < 0.04, 0, np.where(u < 0.05, 65535, np.where(u < 0.07, edge, d)))
    return np.ascontiguousarray(np.clip(d, 0, 65535).astype(np.uint16))


def window_counts(pre):
    """pre: the label map before the median -> cum int [9, H, W]: cum[b, y, x] = pixels of the replicate-bordered 5 x 5 window at (y, x)
    whose label value is <= the b-th value of LABEL_VALUES."""
    H, W = pre.shape
    p = np.pad(R.label_to_bin(pre), 2, mode="edge")
    cnt = np.zeros((9, H, W), np.int64)
    for dy in range(5):
        for dx in range(5):
            w = p[dy:dy + H, dx:dx + W]
            for b in range(9):
                cnt[b] += w == b
    return np.cumsum(cnt, 0)


def median_of_counts(cum, rank=12):
    """the label whose position in the sorted window is `rank` (12 = the median of 25): the first value with more than `rank` pixels at or below it"""
    return R.bin_to_label((cum > rank).argmax(0))


def depth_coverage(pre):
    """What an image asks of the counting median.  -> dict:
    distinct [10]   histogram of the number of distinct label values per window (index = the number);
    le13 [9]        per median value v (ascending): windows whose median is v with #(<= v) == 13 -- one pixel fewer and the median moves up;
    lt12 [9]        per median value v: windows whose median is v with #(< v) == 12 -- one pixel more and the median moves down;
    equal_neighbours  share of horizontally adjacent pixel pairs inside the r = 5 frame with equal labels."""
    cum = window_counts(pre)
    H, W = pre.shape
    per = np.diff(cum, axis=0, prepend=0)
    med = (cum > 12).argmax(0)
    below = np.concatenate([np.zeros((1, H, W), np.int64), cum[:-1]])
    at = np.take_along_axis(cum, med[None], 0)[0]
    under = np.take_along_axis(below, med[None], 0)[0]
    inner = pre[5:H - 6, 5:W - 6]
    return dict(distinct=np.bincount((per > 0).sum(0).reshape(-1), minlength=10),
                le13=np.bincount(med[at == 13], minlength=9), lt12=np.bincount(med[under == 12], minlength=9),
                equal_neighbours=float((inner[:, 1:] == inner[:, :-1]).mean()))


MISPLACEMENTS = ((0, 1), (1, 0), (3, 52))   # (rows, columns): the last is the item step of the depth kernel's pipelined interior-tile loop


def misplaced(pre, shift, seed=0):
    """A planted fault: a tenth of the pixels whose source lies inside the r = 5 frame for every shift take the label (before the median) of
    the pixel `shift` away.  -> (the faulty map, number of planted pixels, number of them whose label changed)."""
    H, W = pre.shape
    dy, dx = shift
    plant = np.zeros((H, W), bool)
    my, mx = max(s[0] for s in MISPLACEMENTS), max(s[1] for s in MISPLACEMENTS)    # the same pixels for every shift
    plant[5:H - 6 - my, 5:W - 6 - mx] = np.random.default_rng([seed, 77]).uniform(0, 1, (H - 11 - my, W - 11 - mx)) < 0.1
    ys, xs = np.nonzero(plant)
    out = pre.copy()
    out[ys, xs] = pre[ys + dy, xs + dx]
    return out, len(ys), int((out != pre).sum())


# ---- colour ----------------------------------------------------------------------------------------------------------------------------
COLOR_KINDS = ("noise", "smooth", "extreme", "faint", "cross")


def color_image(rng, H, W, kind):
    """u8 [H, W, 3] of one family; gray contexts take one plane (gray_plane)."""
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "smooth":   # gradients strong enough to pass the weak threshold, low-pass so that votes reach 5 of 9
        a = rng.uniform(0, 255, (H // 8 + 2, W // 8 + 2, 3))
        a = np.kron(a, np.ones((8, 8, 1)))[:H, :W]
        return np.ascontiguousarray(np.clip(a + rng.normal(0, 3, a.shape), 0, 255).astype(np.uint8))
    if kind == "extreme":  # saturating blocks: Sobel outputs reach +-1020, equal channel magnitudes (first-channel precedence)
        a = (rng.integers(0, 2, (H // 4 + 1, W // 4 + 1, 1)) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(np.kron(a, np.ones((4, 4, 1), np.uint8))[:H, :W], 3, axis=2))
    if kind == "faint":    # gradient magnitudes around the weak threshold: 128 + N(0, sigma), sigma per 24 x 24 cell (one sigma alone leaves one side of the threshold thin)
        sigma = rng.choice(np.array([4.0, 6.0, 8.0]), (-(-H // CELL), -(-W // CELL)))
        a = 128.0 + rng.normal(0, 1, (H, W, 3)) * _per_cell(sigma, H, W)[:, :, None]
        return np.ascontiguousarray(np.clip(np.rint(a), 0, 255).astype(np.uint8))
    if kind == "cross":    # channel 1 = channel 0 transposed: equal magnitudes, other orientations; which channel wins a tie decides the label
        n = max(H, W)
        lv = rng.integers(0, 2, (n // 6 + 1, n // 6 + 1))
        s = np.kron(np.where(lv > 0, 200, 56).astype(np.uint8), np.ones((6, 6), np.uint8))[:n, :n]
        return np.ascontiguousarray(np.stack([s[:H, :W], s.T[:H, :W], np.full((H, W), 128, np.uint8)], 2))
    raise ValueError(kind)


def gray_plane(bgr):
    """the plane a gray context is given, and the BGR image the oracle sees for it"""
    g = np.ascontiguousarray(bgr[:, :, 0])
    return g, np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def color_coverage(bgr, weak_threshold=10.0):
    """What an image asks of the colour quantiser's compares.  -> dict of pixel counts over the interior (the border row and column get no label):
    at, below, above   strongest squared magnitude == weak_threshold ** 2, within 4 below it, within 4 above it;
    vote4, vote5       pixels above the threshold whose best 3 x 3 vote count is exactly 4 (no label) / exactly 5 (the weakest label);
    tied               two channels tie for the strongest magnitude above the threshold and their own orientation labels differ."""
    q, mag, qu = o.quantized_orientations(bgr, weak_threshold)
    dx, dy = o.sobel3(o.gaussian7(bgr))
    m3 = dx.astype(np.int64) ** 2 + dy.astype(np.int64) ** 2
    top = m3.max(2)
    assert np.array_equal(top.astype(np.float32), mag)
    H, W = top.shape
    thr = int(round(weak_threshold * weak_threshold))
    assert thr == np.float32(weak_threshold) * np.float32(weak_threshold)
    lab = qu & 7
    votes = np.zeros((8, H - 2, W - 2), np.int64)
    for sy in range(3):
        for sx in range(3):
            w = lab[sy:sy + H - 2, sx:sx + W - 2]
            for b in range(8):
                votes[b] += w == b
    best = votes.max(0)
    ti, strong = top[1:-1, 1:-1], top[1:-1, 1:-1] > thr
    # the counter's own reading of the rule reproduces the oracle's labels, or its counts mean nothing
    assert np.array_equal(np.where(strong & (best >= 5), 1 << votes.argmax(0), 0).astype(np.uint8), q[1:-1, 1:-1])
    own = o.orientation_labels(dx, dy) & 7
    tied = np.zeros((H, W), bool)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        tied |= (m3[..., a] == top) & (m3[..., b] == top) & (own[..., a] != own[..., b])
    return dict(at=int((ti == thr).sum()), below=int(((ti >= thr - 4) & (ti < thr)).sum()), above=int(((ti > thr) & (ti <= thr + 4)).sum()),
                vote4=int((strong & (best == 4)).sum()), vote5=int((strong & (best == 5)).sum()), tied=int((tied[1:-1, 1:-1] & strong).sum()))


# ---- the frames of tests/test_gpu_quantizer_images.py ------------------------------------------------------------------------------------
# name, W, H, modalities, T, difference_threshold, frames, how, row_pad, env, gray, table
#
# Sizes: the smallest a context accepts (every level a multiple of its T, rows * cols a multiple of 16) that leave a ragged last tile against
# 64 columns and 16 / 32 rows and hold interior depth tiles (the pipelined loop: y0 >= 7, y0 + 33 < H - 6, x0 >= 7, x0 + 65 < W - 6).
#   208 x 112, T = (4, 8): 3 * 64 + 16 columns, 3 * 32 + 16 rows; interior tiles at x0 = 64, 128 and y0 = 32, 64; level 1 is 104 x 56.
#   200 x 120, T = (5,):   3 * 64 + 8 columns, 3 * 32 + 24 rows (7 * 16 + 8); one level, depth only.
#   240 x 160, T = (5, 8, 10): three levels (k_nn_down2, two pyrDown steps).  With these T every size is a multiple of 80, so no height is
#                          ragged against 16 rows; 160 rows leave level 1 (120 x 80) ragged against 32 and level 2 (60 x 40) against both.
#   80 x 80,   T = (5,):   no interior tile, 64 + 16 columns, 2 * 32 + 16 rows.
RGBD = ("ColorGradient", "DepthNormal")
PATHS = [
    ("match_host_frame", 208, 112, RGBD, (4, 8), 50, 1, "match", 0, {}, False, "uniform"),               # k_small_depth_color, streamed rows
    ("match_host_frame_high", 208, 112, RGBD, (4, 8), 200, 1, "match", 0, {}, False, "high"),
    ("enqueue_one", 208, 112, RGBD, (4, 8), 50, 1, "enqueue", 0, {}, False, "high"),
    ("enqueue_two", 208, 112, RGBD, (4, 8), 200, 2, "enqueue", 0, {}, False, "uniform"),
    ("plain_kernels_one", 208, 112, RGBD, (4, 8), 50, 1, "enqueue", 0, {"LMX_NO_SMALL_CHAIN": "1"}, False, "uniform"),   # k_depth_quantize, k_color_quantize
    ("plain_kernels_two", 208, 112, RGBD, (4, 8), 200, 2, "enqueue", 0, {"LMX_NO_SMALL_CHAIN": "1"}, False, "high"),
    ("batch_of_nine", 208, 112, RGBD, (4, 8), 50, 9, "enqueue", 0, {}, False, "uniform"),                # n >= 8: tiles placed by frame, the tall colour tile
    ("batch_of_nine_tile16", 208, 112, RGBD, (4, 8), 50, 9, "enqueue", 0, {"LMX_COLOR_TILE": "16"}, False, "high"),
    ("two_frames_tile32", 208, 112, RGBD, (4, 8), 50, 2, "enqueue", 0, {"LMX_COLOR_TILE": "32"}, False, "uniform"),
    ("row_padded", 208, 112, RGBD, (4, 8), 200, 2, "match_batch", 24, {}, False, "uniform"),
    ("row_padded_plain", 208, 112, RGBD, (4, 8), 50, 3, "match_batch", 10, {"LMX_NO_SMALL_CHAIN": "1"}, False, "high"),
    ("gray_context", 208, 112, RGBD, (4, 8), 50, 1, "match", 0, {}, True, "uniform"),
    ("gray_context_long_form", 208, 112, RGBD, (4, 8), 201, 1, "match", 0, {}, True, "high"),            # the 64-bit form fused with the one-plane colour tile
    ("gray_batch_of_nine", 208, 112, RGBD, (4, 8), 201, 9, "enqueue", 0, {}, True, "uniform"),
    ("long_form_201", 208, 112, RGBD, (4, 8), 201, 2, "enqueue", 0, {}, False, "uniform"),               # the 64-bit kernel
    ("long_form_201_plain", 208, 112, RGBD, (4, 8), 201, 1, "enqueue", 0, {"LMX_NO_SMALL_CHAIN": "1"}, False, "high"),
    ("colour_only", 208, 112, ("ColorGradient",), (4, 8), 50, 2, "match_batch", 6, {}, False, "uniform"),
    ("depth_only_one_level", 200, 120, ("DepthNormal",), (5,), 50, 2, "enqueue", 0, {}, False, "uniform"),
    ("depth_only_one_level_high", 200, 120, ("DepthNormal",), (5,), 200, 1, "match", 6, {}, False, "high"),
    ("three_levels", 240, 160, RGBD, (5, 8, 10), 50, 2, "enqueue", 0, {}, False, "uniform"),             # k_nn_down2, two pyrDown steps on noise
    ("three_levels_nine", 240, 160, RGBD, (5, 8, 10), 200, 9, "enqueue", 0, {}, False, "high"),
    ("no_interior_tile", 80, 80, ("DepthNormal",), (5,), 50, 3, "enqueue", 6, {}, False, "uniform"),
    ("no_interior_tile_high", 80, 80, ("DepthNormal",), (5,), 201, 1, "match", 0, {}, False, "high"),
]
DIST = 2000
MATCH_THRESHOLD = 90.0


def path_frames(path):
    """The frames of one PATHS row, all different: -> list (per frame) of (depth u16 or None, bgr u8 or None, colour family)."""
    name, W, H, mods, T, thr, frames = path[:7]
    k = [p[0] for p in PATHS].index(name)
    out = []
    for f in range(frames):
        depth = hostile_depth(H, W, 100 * k + f, DIST) if "DepthNormal" in mods else None
        kind = COLOR_KINDS[(k + f) % len(COLOR_KINDS)]
        bgr = color_image(np.random.default_rng([k, f, 5]), H, W, kind) if "ColorGradient" in mods else None
        out.append((depth, bgr, kind))
    return out


def path_bank(path):
    from linemod_pose_estimation_amd import synth
    name, W, H, mods, T, thr = path[:6]
    bank = synth.make_bank(4, modalities=mods, T=T, seed=71, size_range=(20.0, 34.0))
    if "DepthNormal" in mods:
        dn = mods.index("DepthNormal")
        bank.modalities[dn]["difference_threshold"] = thr
        bank.modalities[dn]["distance_threshold"] = DIST
        bank.normal_lut = normal_table(path[11])
    return bank


def path_sources(path, frames=None):
    """-> (given, seen): per frame the sources a context is handed (gray plane for a gray context, rows padded with non-zero garbage) and the
    sources the oracle sees (contiguous, BGR)."""
    name, W, H, mods = path[:4]
    row_pad, gray = path[8], path[10]
    given, seen = [], []
    k = [p[0] for p in PATHS].index(name)
    for f, (depth, bgr, _) in enumerate(path_frames(path) if frames is None else frames):
        g, s = [], []
        garbage = np.random.default_rng([k, f, 9])
        for m in mods:
            if m == "ColorGradient":
                if gray:
                    src, ref = gray_plane(bgr)
                else:
                    src = ref = bgr
            else:
                src = ref = depth
            if row_pad:
                info = np.iinfo(src.dtype)
                wide = garbage.integers(1, int(info.max) + 1, (H, W + row_pad) + src.shape[2:], dtype=src.dtype)   # never zero
                wide[:, :W] = src
                src = wide[:, :W]
            g.append(src)
            s.append(ref)
        given.append(g)
        seen.append(s)
    return given, seen


TRAIN_KINDS = ("noise", "smooth", "cross")
TRAIN_STRONG = {"noise": 30.0, "smooth": 55.0, "cross": 55.0}   # strong_threshold: blurred noise halved by pyrDown has no 63 / 31 features above 55


def training_view(kind):
    """A 320 x 240 colour view of one family and an object mask (an ellipse, off centre) for the trainer."""
    W, H = 320, 240
    bgr = color_image(np.random.default_rng([TRAIN_KINDS.index(kind), 31]), H, W, kind)
    ys, xs = np.mgrid[0:H, 0:W]
    mask = ((((xs - 171) / 97.0) ** 2 + ((ys - 113) / 71.0) ** 2) < 1.0).astype(np.uint8) * 255
    return bgr, np.ascontiguousarray(mask)
