"""Second, independent restatement (numpy, whole-array formulations) of the stages of cv::linemod::Detector::match
from SURVEY.md Appendix A.  Test infrastructure only: it pins the C++ oracle (oracle/linemod_oracle.cpp), which
is written as per-pixel loops, against a differently structured implementation of the same published algorithm
(the reference itself has no tests or fixtures for this path: SURVEY.md section 4).
Reference call site of the restated path: /root/reference/src/rgbdDetector.cpp:31-34.
"""
import numpy as np

F32 = np.float32


# ---- A.6: the LUT from its generating rule (not from the table) ------------------------------------------
def similarity_lut_from_rule():
    lut = np.zeros(256, np.uint8)
    for ori in range(8):
        for nib in range(16):
            lo = hi = 0
            for j in range(4):
                if nib >> j & 1:
                    d = abs(ori - j)
                    lo = max(lo, max(0, 4 - min(d, 8 - d)))      # low nibble: circular distance
                    hi = max(hi, max(0, 4 - abs(ori - (j + 4))))  # high nibble: NOT circular (upstream asymmetry)
            lut[32 * ori + nib] = lo
            lut[32 * ori + 16 + nib] = hi
    return lut


# ---- A.2 ---------------------------------------------------------------------------------------------------
def gaussian7(img):
    k = np.array([8, 28, 56, 72, 56, 28, 8], np.int64)
    a = img.astype(np.int64)
    if a.ndim == 2:
        a = a[:, :, None]
    p = np.pad(a, ((0, 0), (3, 3), (0, 0)), mode="edge")
    rows = sum(k[i] * p[:, i:i + a.shape[1]] for i in range(7))
    p = np.pad(rows, ((3, 3), (0, 0), (0, 0)), mode="edge")
    out = sum(k[i] * p[i:i + a.shape[0]] for i in range(7))
    out = np.minimum((out + (1 << 15)) >> 16, 255).astype(np.uint8)
    return out.reshape(img.shape)


def sobel3(sm):
    a = sm.astype(np.int32)
    if a.ndim == 2:
        a = a[:, :, None]
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = a.shape[:2]
    def s(dy, dx):
        return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return gx.astype(np.int16).reshape(sm.shape), gy.astype(np.int16).reshape(sm.shape)


def fast_atan2_deg(y, x):
    """vectorised cv::fastAtan2, float32 throughout, same operation order."""
    y = y.astype(F32)
    x = x.astype(F32)
    scale = F32(180 / np.pi)
    p1 = F32(0.9997878412794807) * scale
    p3 = F32(-0.3258083974640975) * scale
    p5 = F32(0.1555786518463281) * scale
    p7 = F32(-0.04432655554792128) * scale
    eps = F32(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    num = np.where(big, ay, ax)
    den = np.where(big, ax, ay) + eps
    c = (num / den).astype(F32)
    c2 = (c * c).astype(F32)
    poly = ((((p7 * c2).astype(F32) + p5).astype(F32) * c2).astype(F32) + p3).astype(F32)
    poly = (((poly * c2).astype(F32) + p1).astype(F32) * c).astype(F32)
    a = np.where(big, poly, (F32(90.0) - poly).astype(F32)).astype(F32)
    a = np.where(x < 0, (F32(180.0) - a).astype(F32), a)
    a = np.where(y < 0, (F32(360.0) - a).astype(F32), a)
    return a.astype(F32)


def quantized_orientations(bgr, weak_threshold=10.0):
    sm = gaussian7(bgr)
    dx, dy = sobel3(sm)
    dx = dx.astype(np.int32)
    dy = dy.astype(np.int32)
    mag3 = dx * dx + dy * dy
    m0, m1, m2 = mag3[..., 0], mag3[..., 1], mag3[..., 2]
    c0 = (m0 >= m1) & (m0 >= m2)
    c1 = ~c0 & (m1 >= m0) & (m1 >= m2)
    sel = np.where(c0, 0, np.where(c1, 1, 2))
    ii, jj = np.indices(sel.shape)
    sx, sy, mag = dx[ii, jj, sel], dy[ii, jj, sel], mag3[ii, jj, sel].astype(F32)
    ang = fast_atan2_deg(sy, sx)
    q = np.clip(np.rint((ang * F32(16.0 / 360.0)).astype(F32)), 0, 255).astype(np.uint8)  # rint = half to even
    q[0, :] = 0
    q[-1, :] = 0
    q[:, 0] = 0
    q[:, -1] = 0
    q[1:-1, 1:-1] &= 7
    H, W = q.shape
    votes = np.zeros((8, H, W), np.int32)
    lab = q & 7
    for dy_ in (-1, 0, 1):
        for dx_ in (-1, 0, 1):
            sh = np.zeros((H, W), np.int64) - 1
            ys = slice(max(0, -dy_), H - max(0, dy_))
            xs = slice(max(0, -dx_), W - max(0, dx_))
            yd = slice(max(0, dy_), H - max(0, -dy_))
            xd = slice(max(0, dx_), W - max(0, -dx_))
            sh[ys, xs] = lab[yd, xd]
            for b in range(8):
                votes[b] += (sh == b)
    best = votes.argmax(0)            # first maximum, like upstream's strict '<' scan
    maxv = votes.max(0)
    out = np.zeros((H, W), np.uint8)
    ok = (mag > F32(weak_threshold) * F32(weak_threshold)) & (maxv >= 5)
    ok[0, :] = ok[-1, :] = False
    ok[:, 0] = ok[:, -1] = False
    out[ok] = (1 << best[ok]).astype(np.uint8)
    return out, mag


# ---- A.3 ---------------------------------------------------------------------------------------------------
def pyrdown(img):
    k = np.array([1, 4, 6, 4, 1], np.int64)
    a = img.astype(np.int64)
    if a.ndim == 2:
        a = a[:, :, None]
    H, W = a.shape[:2]
    p = np.pad(a, ((0, 0), (2, 2), (0, 0)), mode="reflect")
    rows = sum(k[i] * p[:, i:i + W:2][:, :W // 2] for i in range(5))
    p = np.pad(rows, ((2, 2), (0, 0), (0, 0)), mode="reflect")
    out = sum(k[i] * p[i:i + H:2][:H // 2] for i in range(5))
    out = ((out + 128) >> 8).astype(np.uint8)
    return out.reshape((H // 2, W // 2) + img.shape[2:])


# ---- A.4 (with the restatement-defined NORMAL_LUT rule of DESIGN.md) ------------------------------------------
def normal_label(v2, v1):
    cx = 2 * v1 - 19
    cy = 2 * v2 - 19
    a, b = np.abs(cx), np.abs(cy)
    horiz = 2 * a * b < a * a - b * b
    vert = ~horiz & (2 * a * b < b * b - a * a)
    k = np.where(horiz, np.where(cx > 0, 0, 4),
                 np.where(vert, np.where(cy > 0, 2, 6),
                          np.where(cx > 0, np.where(cy > 0, 1, 7), np.where(cy > 0, 3, 5))))
    return (1 << k).astype(np.uint8)


def median5(img):
    p = np.pad(img, 2, mode="edge")
    H, W = img.shape
    st = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)], 0)
    return np.sort(st, 0)[12]


def default_normal_lut():
    """The restatement-defined default NORMAL_LUT[20][20][20]: azimuth sector of the cell centre, nz ignored."""
    v2, v1 = np.indices((20, 20))
    return np.broadcast_to(normal_label(v2, v1), (20, 20, 20)).copy()


def quantized_normals(depth, distance_threshold=2000, difference_threshold=50, normal_lut=None):
    d = depth.astype(np.int64)
    H, W = d.shape
    r = 5
    out = np.zeros((H, W), np.uint8)
    ys, xs = slice(r, H - r - 1), slice(r, W - r - 1)
    c = d[ys, xs]
    A0 = np.zeros_like(c); A1 = np.zeros_like(c); A3 = np.zeros_like(c); b0 = np.zeros_like(c); b1 = np.zeros_like(c)
    for j in (-r, 0, r):
        for i in (-r, 0, r):
            if i == 0 and j == 0:
                continue
            nb = d[r + j:H - r - 1 + j, r + i:W - r - 1 + i]
            delta = nb - c
            f = (np.abs(delta) < difference_threshold).astype(np.int64)
            A0 += f * i * i; A1 += f * i * j; A3 += f * j * j
            b0 += f * i * delta; b1 += f * j * delta
    det = A0 * A3 - A1 * A1
    ddx = A3 * b0 - A1 * b1
    ddy = -A1 * b0 + A0 * b1
    nx = (1150 * ddx).astype(F32)
    ny = (1150 * ddy).astype(F32)
    nz = (-det * c).astype(F32)
    s = np.sqrt(((nx * nx).astype(F32) + (ny * ny).astype(F32)).astype(F32) + (nz * nz).astype(F32)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F32(1.0) / s).astype(F32)
        v1 = ((nx * inv).astype(F32) * F32(10) + F32(10)).astype(F32)
        v2 = ((ny * inv).astype(F32) * F32(10) + F32(10)).astype(F32)
        v3 = ((nz * inv).astype(F32) * F32(20) + F32(20)).astype(F32)
    good = (c < distance_threshold) & (s > 0)
    v1i = np.where(good, v1, 0).astype(np.int64)   # truncation toward zero, values are >= 0
    v2i = np.where(good, v2, 0).astype(np.int64)
    v3i = np.where(good, v3, 0).astype(np.int64)
    # NORMAL_LUT[v3][v2][v1] with C's flat layout; indices past the table (upstream UB) give no label
    lut = (default_normal_lut() if normal_lut is None else np.asarray(normal_lut, np.uint8)).reshape(8000)
    idx = (v3i * 20 + v2i) * 20 + v1i
    lab = np.where(idx < 8000, lut[np.minimum(idx, 7999)], 0).astype(np.uint8)
    out[ys, xs] = np.where(good, lab, 0)
    return median5(out), out


# Per-tuple form of the stage before the median: a pixel of quantizedNormals sees the image only through nine values (its depth and
# the eight neighbours at distance 5), so the stage is a function of that tuple and can be evaluated where no image is at hand --
# at the rounding boundaries of the float chain and at the edges of the integer ranges (tests/depth_cases.py).
TAP_OFFSETS = ((-5, -5), (-5, 0), (-5, 5), (0, -5), (0, 5), (5, -5), (5, 0), (5, 5))   # (j = dy, i = dx) of taps[:, 1:], upstream's order


def _ulps(x, k):
    """float32 array x moved by k units in the last place (k in {-1, 0, 1}; x > 0 where k != 0)."""
    if k == 0:
        return x
    return np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf)).astype(F32)


def normal_bin_of_taps(taps, dist_thr, diff_thr, lut=None, s_ulps=0, inv_ulps=0, detail=False):
    """taps: [n, 9] integers, the pixel's depth then its eight neighbours in TAP_OFFSETS order; dist_thr, diff_thr: scalars or [n].
    -> (bin, idx, ss): the median bin before the median (0 = no label, k + 1 = label 1 << k), the flat NORMAL_LUT index of the
    look-up (-1 where there is none: far pixel, s == 0, index past the table) and the float32 sum of squares.
    int64 accumulation like upstream's `long`, then float32 with numpy's correctly rounded sqrt and divide in the written order.
    s_ulps / inv_ulps move s / inv by that many float32 ulps: the mutants a test must be able to tell from the real thing."""
    t = np.asarray(taps).astype(np.int64).reshape(-1, 9)
    dist = np.broadcast_to(np.asarray(dist_thr, np.int64), t.shape[:1])
    thr = np.broadcast_to(np.asarray(diff_thr, np.int64), t.shape[:1])
    d = t[:, 0]
    A0 = np.zeros_like(d); A1 = np.zeros_like(d); A3 = np.zeros_like(d); b0 = np.zeros_like(d); b1 = np.zeros_like(d)
    for k, (j, i) in enumerate(TAP_OFFSETS):
        delta = t[:, 1 + k] - d
        f = (np.abs(delta) < thr).astype(np.int64)
        A0 += f * (i * i); A1 += f * (i * j); A3 += f * (j * j)
        b0 += f * i * delta; b1 += f * j * delta
    det = A0 * A3 - A1 * A1
    ddx = A3 * b0 - A1 * b1
    ddy = -A1 * b0 + A0 * b1
    nx = (1150 * ddx).astype(F32)
    ny = (1150 * ddy).astype(F32)
    nz = (-det * d).astype(F32)
    ss = (((nx * nx).astype(F32) + (ny * ny).astype(F32)).astype(F32) + (nz * nz).astype(F32)).astype(F32)
    s = np.sqrt(ss).astype(F32)
    pos = s > 0
    s = np.where(pos, _ulps(np.where(pos, s, F32(1)), s_ulps), s).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F32(1.0) / s).astype(F32)
        inv = np.where(pos, _ulps(np.where(pos, inv, F32(1)), inv_ulps), inv).astype(F32)
        v1 = ((nx * inv).astype(F32) * F32(10) + F32(10)).astype(F32)
        v2 = ((ny * inv).astype(F32) * F32(10) + F32(10)).astype(F32)
        v3 = ((nz * inv).astype(F32) * F32(20) + F32(20)).astype(F32)
    good = (d < dist) & pos
    v1i = np.where(good, v1, 0).astype(np.int64)   # truncation toward zero
    v2i = np.where(good, v2, 0).astype(np.int64)
    v3i = np.where(good, v3, 0).astype(np.int64)
    flat = (v3i * 20 + v2i) * 20 + v1i
    look = good & (flat >= 0) & (flat < 8000)
    idx = np.where(look, flat, -1)
    table = (default_normal_lut() if lut is None else np.asarray(lut, np.uint8)).reshape(8000)
    lab = np.where(look, table[np.clip(idx, 0, 7999)], 0).astype(np.uint8)
    bins = label_to_bin(lab)
    if detail:
        return bins, idx, ss, dict(det=det, ddx=ddx, ddy=ddy, far=~(d < dist), v1=v1i, v2=v2i, v3=v3i, good=good,
                                   mask=sum(((np.abs(t[:, 1 + k] - d) < thr).astype(np.int64) << k) for k in range(8)))
    return bins, idx, ss


def label_to_bin(lab):
    """0 -> 0, 1 << k -> k + 1: the order of the label VALUES, which is what the median sorts by."""
    lab = np.asarray(lab, np.uint8)
    out = np.zeros(lab.shape, np.uint8)
    for k in range(8):
        out[lab == (1 << k)] = k + 1
    return out


def bin_to_label(b):
    b = np.asarray(b).astype(np.int64)
    return np.where(b > 0, 1 << np.maximum(b - 1, 0), 0).astype(np.uint8)


# ---- A.5 - A.7 -----------------------------------------------------------------------------------------------
def spread(q, T):
    H, W = q.shape
    out = np.zeros_like(q)
    for r in range(T):
        for c in range(T):
            out[:H - r, :W - c] |= q[r:, c:]
    return out


def response_maps(spr, lut=None):
    lut = similarity_lut_from_rule() if lut is None else lut
    lo, hi = spr & 15, spr >> 4
    return np.stack([np.maximum(lut[32 * o + lo], lut[32 * o + 16 + hi]) for o in range(8)], 0)


def linearize(rmap, T):
    H, W = rmap.shape
    return np.stack([rmap[r0::T, c0::T].reshape(-1) for r0 in range(T) for c0 in range(T)], 0)


# ---- A.8 - A.10 (python loops: small cases only) ----------------------------------------------------------------
def _lm_read(lm_o, base, n):
    """flat read of `n` elements starting at `base` of one orientation's [T*T, cells] matrix; zero past the end."""
    flat = lm_o.reshape(-1)
    out = np.zeros(n, np.int64)
    hi = min(len(flat), base + n)
    if hi > base:
        out[:hi - base] = flat[base:hi]
    return out


def similarity(lm, size_wh, T, templ_wh, feats):
    w, h = size_wh
    Wc, Hc = w // T, h // T
    wf, hf = (templ_wh[0] - 1) // T + 1, (templ_wh[1] - 1) // T + 1
    positions = (Hc - hf) * Wc + (Wc - wf) + 1
    dst = np.zeros(Wc * Hc, np.int64)
    for x, y, label in feats:
        if x < 0 or x >= w or y < 0 or y >= h:
            continue
        base = ((y % T) * T + x % T) * (Wc * Hc) + (y // T) * Wc + x // T
        if positions > 0:
            dst[:positions] += _lm_read(lm[label], base, positions)
    return (dst & 255).astype(np.uint8).reshape(Hc, Wc), positions


def similarity_local(lm, size_wh, T, feats, cx, cy):
    w, h = size_wh
    Wc, Hc = w // T, h // T
    ox, oy = (int(cx / T) - 8) * T, (int(cy / T) - 8) * T   # int(): C++ truncation toward zero
    dst = np.zeros((16, 16), np.int64)
    for x, y, label in feats:
        x, y = x + ox, y + oy
        if x < 0 or y < 0 or x >= w or y >= h:
            continue
        base = ((y % T) * T + x % T) * (Wc * Hc) + (y // T) * Wc + x // T
        for r in range(16):
            dst[r] += _lm_read(lm[label], base + r * Wc, 16)
    return (dst & 255).astype(np.uint8)


def raw_threshold(nf, thr):
    return int(F32(2 * nf) + (F32(thr) / F32(100.0)) * F32(2 * nf) + F32(0.5))


def quantize_pyramid(bank, sources):
    """The label images of Detector::match, [level][modality] -> uint8 (H_l, W_l): quantize() and pyrDown() of every modality."""
    L, M = len(bank.T), len(bank.modalities)
    color = [None] * M
    quant = [None] * M
    H, W = sources[0].shape[:2]
    out = []
    for l in range(L):
        if l > 0:
            H, W = H // 2, W // 2
        for m, mod in enumerate(bank.modalities):
            if mod["type"] == "ColorGradient":
                color[m] = np.ascontiguousarray(sources[m]) if l == 0 else pyrdown(color[m])
                q, _ = quantized_orientations(color[m], mod["weak_threshold"])
            else:
                q = quantized_normals(np.ascontiguousarray(sources[m]), mod["distance_threshold"], mod["difference_threshold"],
                                      getattr(bank, "normal_lut", None))[0] \
                    if l == 0 else quant[m][::2, ::2][:H, :W].copy()
            quant[m] = q
        out.append(list(quant))
    return out


def match(bank, sources, threshold):
    """Whole Detector::match for a TemplateBank; returns pre-sort matches as tuples
    (x, y, similarity(float32), class_id, template_id) in upstream insertion order."""
    return match_labels(bank, quantize_pyramid(bank, sources), threshold)


def _local_sums(flat8, n, Wc, size_wh, T, feats, cx, cy):
    """similarity_local for all features at once: flat8 = one modality's [8, n] memories read flat (zero past the end)."""
    w, h = size_wh
    if not len(feats):
        return np.zeros((16, 16), np.int64)
    f = np.asarray(feats, np.int64).reshape(-1, 3)
    x, y = f[:, 0] + (int(cx / T) - 8) * T, f[:, 1] + (int(cy / T) - 8) * T    # int(): C++ truncation toward zero
    ok = (x >= 0) & (y >= 0) & (x < w) & (y < h)
    x, y, lab = x[ok], y[ok], f[ok, 2]
    base = ((y % T) * T + x % T) * n + (y // T) * Wc + x // T
    idx = base[:, None, None] + np.arange(16)[None, :, None] * Wc + np.arange(16)[None, None, :]
    inside = (idx >= 0) & (idx < T * T * n)
    v = np.where(inside, flat8[lab[:, None, None], np.clip(idx, 0, T * T * n - 1)], 0)
    return v.sum(0).astype(np.int64)


def match_labels(bank, labels, threshold, class_ids=(), mutant=None, lut=None, stats=None):
    """Detector::match from the label images on: labels[level][modality] uint8 (H_l, W_l).  threshold: a float, or a mapping class id ->
    float (classes it lacks are not matched).  -> pre-sort matches (x, y, similarity(float32), class_id, template_id) in upstream insertion
    order; stats (a dict) gets "candidates".  lut: the response table instead of the rule's.  mutant: a deliberately wrong variant a test
    must be able to tell from the real thing -- "coarse_ge" (>= at the coarse test), "last_max" (the last maximum of a patch), "refine_le"
    (<= at the refinement test), "u8_wrap" (the sum over the modalities wraps at 256)."""
    L, M = len(bank.T), len(bank.modalities)
    H0, W0 = np.shape(labels[0][0])
    sizes = [(W0 >> l, H0 >> l) for l in range(L)]
    lms = []
    for l in range(L):
        lv = []
        for m in range(M):
            r = response_maps(spread(np.asarray(labels[l][m], np.uint8), bank.T[l]), lut)
            lv.append(np.stack([linearize(r[o], bank.T[l]) for o in range(8)], 0))
        lms.append(lv)
    out = []
    n_cand = 0
    per = L * M
    order = sorted(bank.classes, key=lambda c: c[0])
    if len(class_ids):
        by_id = {c[0]: c for c in order}
        order = [by_id[c] for c in class_ids if c in by_id]
    for cid, templates, feats in order:
        if isinstance(threshold, dict):
            if cid not in threshold:
                continue
            thr = threshold[cid]
        else:
            thr = threshold
        for tid in range(templates.shape[0] // per):
            tp = [templates[tid * per + k] for k in range(per)]
            fl = [[tuple(int(v) for v in f) for f in feats[t[3]:t[3] + t[4]]] for t in tp]
            Tl = bank.T[-1]
            w, h = sizes[-1]
            tot = np.zeros((h // Tl, w // Tl), np.int64)
            nf = 0
            for m in range(M):
                k = (L - 1) * M + m
                s, _ = similarity(lms[-1][m], sizes[-1], Tl, (tp[k][0], tp[k][1]), fl[k])
                tot += s
                nf += len(fl[k])
            if mutant == "u8_wrap":
                tot &= 255
            rt = raw_threshold(nf, thr)
            off = Tl // 2 + (Tl % 2 - 1)
            rr, cc = np.nonzero(tot >= rt if mutant == "coarse_ge" else tot > rt)
            cands = [[int(c) * Tl + off, int(r) * Tl + off, F32(F32(int(tot[r, c])) * F32(100.0) / F32(4 * nf)) + F32(0.5)] for r, c in zip(rr, cc)]
            n_cand += len(cands)
            for l in range(L - 2, -1, -1):
                T = bank.T[l]
                w, h = sizes[l]
                n = (w // T) * (h // T)
                flat = [lms[l][m].reshape(8, -1) for m in range(M)]
                border, off = 8 * T, T // 2 + (T % 2 - 1)
                max_x, max_y = w - tp[l * M][0] - border, h - tp[l * M][1] - border
                nf2 = sum(len(fl[l * M + m]) for m in range(M))
                keep = []
                for x, y, _ in cands:
                    x, y = 2 * x + 1, 2 * y + 1
                    x, y = max(x, border), max(y, border)
                    x, y = min(x, max_x), min(y, max_y)
                    tot2 = np.zeros((16, 16), np.int64)
                    for m in range(M):
                        # one modality's patch wraps at 256 like upstream's uchar, the sum over modalities is a ushort
                        tot2 += _local_sums(flat[m], n, w // T, sizes[l], T, fl[l * M + m], x, y) & 255
                    best = int(tot2.max())
                    br, bc = -1, -1
                    if best > 0:
                        hits = np.flatnonzero(tot2.reshape(-1) == best)
                        br, bc = divmod(int(hits[-1] if mutant == "last_max" else hits[0]), 16)   # first maximum in row-major order
                    nx = (int(x / T) - 8 + bc) * T + off
                    ny = (int(y / T) - 8 + br) * T + off
                    sim = F32(F32(best) * F32(100.0) / F32(4 * nf2))
                    if not (sim <= F32(thr) if mutant == "refine_le" else sim < F32(thr)):
                        keep.append([nx, ny, sim])
                cands = keep
            out += [(x, y, F32(s), cid, tid) for x, y, s in cands]
    if stats is not None:
        stats["candidates"] = n_cand
    return out


# ---- node-side steps in front of match() (lmx_ctx_upload_raw; the oracle's pre_color / pre_depth) ----------------------------------------
def pre_color(src, crop_xy, size_wh, blur3=True):
    """(MONO8 -> BGR) + GaussianBlur 3x3 (sigma 0: [1 2 1] / 4 per axis, on 8U exactly (sum + 8) >> 4, BORDER_REFLECT_101) on the FULL
    frame, then the crop.  src: u8 HxW or HxWx3 -> u8 [H, W, 3]."""
    img = np.asarray(src, np.uint8)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    if blur3:
        p = np.pad(img.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="reflect")
        h = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
        v = h[:-2] + 2 * h[1:-1] + h[2:]
        img = ((v + 8) >> 4).astype(np.uint8)
    (cx, cy), (W, H) = crop_xy, size_wh
    return np.ascontiguousarray(img[cy:cy + H, cx:cx + W])


def pre_depth(z, crop_xy, size_wh):
    """convertTo(CV_16UC1, 1000.0) of float metres: the float32 product, cvRound (half to even), saturate to u16; NaN, Inf and products
    outside (-2^31, 2^31) give 0 (x86's integer indefinite, saturated)."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(z, np.float32) * np.float32(1000.0)
        assert v.dtype == np.float32
        ok = (v > np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
        r = np.clip(np.rint(np.where(ok, v, np.float32(0)).astype(np.float64)), 0, 65535)
    (cx, cy), (W, H) = crop_xy, size_wh
    return np.ascontiguousarray(np.where(ok, r, 0).astype(np.uint16)[cy:cy + H, cx:cx + W])


def _z_with_product(target, span=4):
    """float32 z near target / 1000 whose float32 product z * 1000.f is exactly `target`, or None."""
    z0 = np.float32(np.float64(target) / 1000.0)
    cand = [z0]
    lo = hi = z0
    for _ in range(span):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        cand += [lo, hi]
    for z in cand:
        if np.float32(z) * np.float32(1000.0) == np.float32(target) and np.float64(np.float32(target)) == np.float64(target):
            return np.float32(z)
    return None


def pre_depth_special_values(k_range=range(0, 3000, 7)):
    """The float32 inputs at which float-metre -> u16-millimetre conversion can go wrong.  -> (table float32 [n], n_even, n_odd): the
    number of z found whose product is exactly k + 0.5 with k even / odd (ties: half to even decides)."""
    up, dn = (lambda z: np.nextafter(np.float32(z), np.float32(np.inf))), (lambda z: np.nextafter(np.float32(z), np.float32(-np.inf)))
    out, n_even, n_odd = [], 0, 0
    for k in k_range:
        z = _z_with_product(k + 0.5)
        if z is None:
            continue
        if (k % 2 == 0 and n_even >= 40) or (k % 2 == 1 and n_odd >= 40):
            continue
        n_even, n_odd = n_even + (k % 2 == 0), n_odd + (k % 2 == 1)
        out += [z, up(z), dn(z)]
        if k < 200:
            out += [-z, -up(z), -dn(z)]                      # negative ties and their neighbours
    out += [-0.0, 0.0, -1e-4, -4e-4, -4.9e-4, -6e-4, -1e-3, -1.4e-3, -1.6e-3, -0.3]                          # small negatives, -0.0
    out += [1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 1.17549435e-38]                                     # denormals, the smallest normal
    for target in (65534.5, 65535.0, 65535.5, 70000.0):     # the saturation: the z whose product is the target where one exists (not
        z = _z_with_product(target)                          # every float is a product z * 1000.f), and the z on either side of it
        if z is None:
            z = np.float32(target / 1000.0)
            while np.float32(z) * np.float32(1000.0) > np.float32(target):
                z = dn(z)
        out += [z, up(z), dn(z)]
    z = np.float32(2147483.648)
    while np.float32(z) * np.float32(1000.0) >= np.float32(2147483648.0):
        z = dn(z)
    while np.float32(up(z)) * np.float32(1000.0) < np.float32(2147483648.0):
        z = up(z)
    out += [z, up(z), -z, -up(z)]                            # the largest product below 2^31, the first one that reaches it
    out += [3e38, -3e38, 3.5e35, np.inf, -np.inf, np.nan]   # products that overflow to Inf
    return np.asarray(out, np.float32), n_even, n_odd


def pre_special_frames(SW, SH, seed):
    """Raw frames for the node-side steps: a BGR noise frame with runs of 0 and 255 (the blur's rounding and its reflected border see
    extremes next to noise) and a float32 depth plane tiled with pre_depth_special_values().  -> (bgr, z, table, n_even, n_odd)."""
    rng = np.random.default_rng(seed)
    bgr = rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    for _ in range(60):
        y, x, n, c = int(rng.integers(0, SH)), int(rng.integers(0, SW)), int(rng.integers(2, 40)), int(rng.integers(0, 4))
        bgr[y, x:x + n, slice(0, 3) if c == 3 else slice(c, c + 1)] = rng.choice([0, 255])   # all channels, or one
    bgr[[0, 1, -2, -1], ::3] = 255       # extremes on the rows and columns the reflected border reads twice
    bgr[::5, [0, 1, -2, -1]] = 0
    table, n_even, n_odd = pre_depth_special_values()
    z = table[(np.arange(SH)[:, None] * SW + np.arange(SW)[None, :]) % len(table)]
    return np.ascontiguousarray(bgr), np.ascontiguousarray(z), table, n_even, n_odd


# ---- the device bank's tables (csrc/lmx_bank_tables.hpp), from the bank's flat arrays ----------------------------------------
# What the scoring and refinement kernels are told about a bank, restated from the formats' documentation with whole-array numpy:
# tests/test_bank_tables.py decodes the library's tables (lmx_debug_bank_tables) and compares them with these.  `g` is one pyramid
# level's geometry as a dict of the LevelGeom fields (GEOM_FIELDS, the order of the hook's summary words).
GEOM_FIELDS = ("W", "H", "T", "Wc", "Hc", "cells", "ori_stride", "mod_stride", "zero_off", "nib_ori_stride", "nib_mod_stride", "nib_zero_off",
               "ls_stride", "ls_zero_off", "ls_bands", "ls_band_stride")
FEAT_STRIDE, SB_GROUPS, SB_BLOCK, SB_MAX_BLOCKS = 64, 5, 16, 6
NONE = np.int64(1) << 40   # "no entry" in a padded multiset: above every 32-bit table entry, so it sorts last


def shard_features(bank, rank, world):
    """The templates shard `rank` of `world` holds, classes in key order, as padded arrays: class_index, template_id [G]; wh [G, L, 2];
    count [L, G, M]; x, y, label, valid [L, G, M, 64] (valid = the feature exists)."""
    L, M = len(bank.T), len(bank.modalities)
    ranges = bank.shard(rank, world)
    ci_all, tid_all, wh_all, per_level = [], [], [], [[] for _ in range(L)]
    for ci, (cid, t, f) in enumerate(sorted(bank.classes, key=lambda c: c[0])):
        b, e = ranges[cid]
        t = np.asarray(t, np.int64).reshape(-1, L * M, 5)[b:e]
        f = np.concatenate([np.asarray(f, np.int64).reshape(-1, 3), np.zeros((1, 3), np.int64)])   # the last row stands for "no feature"
        ci_all.append(np.full(e - b, ci)); tid_all.append(np.arange(b, e)); wh_all.append(t[:, ::M, :2])
        for l in range(L):
            rows = t[:, l * M:(l + 1) * M]
            valid = np.arange(FEAT_STRIDE) < rows[..., 4, None]
            per_level[l].append((f[np.where(valid, rows[..., 3, None] + np.arange(FEAT_STRIDE), len(f) - 1)], valid, rows[..., 4]))
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, np.int64)
    ff = np.stack([cat([p[0] for p in lv], (0, M, FEAT_STRIDE, 3)) for lv in per_level])
    return dict(class_index=cat(ci_all, (0,)), template_id=cat(tid_all, (0,)), wh=cat(wh_all, (0, L, 2)), x=ff[..., 0], y=ff[..., 1], label=ff[..., 2],
                valid=np.stack([cat([p[1] for p in lv], (0, M, FEAT_STRIDE)) for lv in per_level]).astype(bool),
                count=np.stack([cat([p[2] for p in lv], (0, M)) for lv in per_level]))


def linear_index(g, x, y):
    """accessLinearMemory: the element of a feature at (x, y) in one orientation's [T * T][Hc * Wc] linear memories, placement 0."""
    T = g["T"]
    return ((y % T) * T + x % T) * g["cells"] + (y // T) * g["Wc"] + x // T


def template_positions(g, w, h):
    """Placements of a w x h template on the level's grid of cells (C++ integer division: a width of 0 spans one cell)."""
    wf, hf = np.where(w > 0, (w - 1) // g["T"] + 1, 1), np.where(h > 0, (h - 1) // g["T"] + 1, 1)
    return np.maximum(0, (g["Hc"] - hf) * g["Wc"] + (g["Wc"] - wf) + 1)


def coarse_address(g, x, y, label, valid):
    """Where the scoring kernels read a coarsest-level feature in ONE modality's nibble-packed memories (two elements per byte, orientation
    blocks nib_ori_stride apart): -> (byte offset of the aligned dword that holds element e0, nibble of e0 inside it).  A feature outside the
    image (upstream similarity() skips it) and every padding entry point at the block's zero run, nibble 0."""
    e0 = linear_index(g, x, y)
    inside = valid & (x < g["W"]) & (y < g["H"])
    return np.where(inside, label * g["nib_ori_stride"] + 4 * (e0 // 8), g["nib_zero_off"] // 4 * 4), np.where(inside, e0 % 8, 0)


def feat_entries(g, x, y, label, valid, count):
    """k_refine's rows [.., 64] as (off, x, y): label << 29 over the flat element index, or over row << 12 | column of the banded image's
    matrix (row = grid * Hc + cell row); padding = the level's zero run, and entry 63's y = the row's feature count."""
    T = g["T"]
    low = (((y % T) * T + x % T) * g["Hc"] + y // T) << 12 | x // T if g["ls_bands"] else linear_index(g, x, y)
    off = np.where(valid, label << 29 | low, g["ls_zero_off"])
    ex, ey = np.where(valid, x, 0), np.where(valid, y, 0)
    ey[..., FEAT_STRIDE - 1] = count
    return off, ex, ey


def coarse_group_plan(nibble, valid):
    """How a template's coarsest-level features (nibble [G, n], valid [G, n]: all modalities) form groups of three.  Full triples of one
    nibble class come first, taken round robin over the classes 0..7; then one group per class that has leftovers, in class order.
    -> n_fast [G]; group_class, group_real [G, 30] (-1 / 0 behind the template's groups); n_groups [G]."""
    G = nibble.shape[0]
    cnt = np.stack([(valid & (nibble == k)).sum(1) for k in range(8)], 1)
    full, left = cnt // 3, cnt % 3
    cap = SB_GROUPS * SB_MAX_BLOCKS + 8
    group_class, group_real, n = np.full((G, cap), -1), np.zeros((G, cap), np.int64), np.zeros(G, np.int64)
    rows = np.arange(G)
    for r in range(int(full.max()) if G else 0):
        for k in range(8):
            sel = full[:, k] > r
            group_class[rows[sel], n[sel]] = k; group_real[rows[sel], n[sel]] = 3
            n += sel
    n_fast = n.copy()
    for k in range(8):
        sel = left[:, k] > 0
        group_class[rows[sel], n[sel]] = k; group_real[rows[sel], n[sel]] = left[sel, k]
        n += sel
    return n_fast, group_class, group_real, n


# ---- A.11: the trainer's extractTemplate, brute force ------------------------------------------------------------------
TRAIN_NO_ZERO = float(1 << 28)   # the distance where an image has no zero pixel at all (upstream: the transform's initial value)


def erode3(mask):
    """cv::erode, 3x3 rectangle, BORDER_REPLICATE: the minimum over the nine shifted copies of the edge-padded image."""
    p = np.pad(np.asarray(mask, np.uint8), 1, mode="edge")
    H, W = mask.shape
    return np.min([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)


def chessboard_distance(img):
    """distanceTransform(DIST_C): per pixel the minimum of max(|dx|, |dy|) over ALL zero pixels of img, no propagation."""
    H, W = img.shape
    zy, zx = np.nonzero(img == 0)
    if len(zy) == 0:
        return np.full((H, W), TRAIN_NO_ZERO, F32)
    y, x = np.mgrid[0:H, 0:W]
    d = np.maximum(np.abs(y[:, :, None] - zy[None, None, :]), np.abs(x[:, :, None] - zx[None, None, :])).min(axis=2)
    return d.astype(F32)


def select_scattered(xs, ys, labels, num_features, distance):
    """selectScatteredFeatures: candidates in ranked order; a candidate is kept when it is at least `distance` (float32) away from every kept
    one; at the end of the list the distance drops by one and the walk restarts -> int32 [num_features, 3]."""
    kept = []
    distance = F32(distance)
    i = 0
    while len(kept) < num_features:
        dsq = F32(distance * distance)
        if all(F32((int(xs[i]) - kx) ** 2 + (int(ys[i]) - ky) ** 2) >= dsq for kx, ky, _ in kept):
            kept.append((int(xs[i]), int(ys[i]), int(labels[i])))
        i += 1
        if i == len(xs):
            i = 0
            distance = F32(distance - F32(1.0))
    return np.asarray(kept, np.int32).reshape(-1, 3)


def _bin_of(q):
    return int(q).bit_length() - 1


def extract_color(angle, magnitude, mask, num_features, strong_threshold):
    """ColorGradientPyramid::extractTemplate -> features or None."""
    angle, magnitude = np.asarray(angle, np.uint8), np.asarray(magnitude, F32)
    ok = (angle > 0) & (magnitude > F32(strong_threshold) * F32(strong_threshold))
    if mask is not None:
        m = np.asarray(mask, np.uint8)
        ok &= (m.astype(np.int32) - erode3(m).astype(np.int32)) > 0         # the mask's inner contour
    ys, xs = np.nonzero(ok)                                                 # raster order
    if len(ys) < num_features:
        return None
    order = np.argsort(-magnitude[ys, xs], kind="stable")                   # high magnitude first, ties in raster order
    ys, xs = ys[order], xs[order]
    labels = [_bin_of(angle[y, x]) for y, x in zip(ys, xs)]
    return select_scattered(xs, ys, labels, num_features, F32(len(ys) // num_features + 1))


def extract_depth(normal, mask, num_features, extract_threshold):
    """DepthNormalPyramid::extractTemplate -> features or None."""
    normal = np.asarray(normal, np.uint8)
    inside = np.ones(normal.shape, bool) if mask is None else erode3(erode3(np.asarray(mask, np.uint8))) > 0
    score = np.zeros(normal.shape, F32)
    label = np.full(normal.shape, -1)
    for k in range(8):
        here = inside & (normal == (1 << k))
        d = chessboard_distance(np.where(inside, normal & (1 << k), 0))     # 255 carries every bit: it is no zero pixel of any label's image
        score[here], label[here] = d[here], k
    ok = (label >= 0) & (score >= F32(extract_threshold))
    ys, xs = np.nonzero(ok)
    if len(ys) < num_features:
        return None
    lab = label[ys, xs]
    counts = np.bincount(lab, minlength=8)
    s = (score[ys, xs] / counts[lab].astype(F32)).astype(F32)
    order = np.argsort(-s, kind="stable")
    ys, xs, lab = ys[order], xs[order], lab[order]
    distance = F32(np.sqrt(F32(int(inside.sum()))) / np.sqrt(F32(num_features)) + F32(1.5))
    return select_scattered(xs, ys, lab, num_features, distance)


# ---- the spread and response buffers of one (frame, modality), every byte (csrc/lmx_bank_tables.hpp: LevelGeom) ---------------------------
# What the refinement and scoring kernels may read, restated from the layout comments: the payload, its second copy in the banded form, and
# every pad, which must read as zero.  Each builder returns the expected bytes of one block and, per byte, which kind of place it is, so that
# first_difference can name the place of a wrong byte.  tests/test_buffer_layout_host.py checks the builders against the debug reads' own
# un-banding and unpacking and against k_refine's addressing; tests/test_gpu_buffer_bytes.py compares the device's allocations with them.
BYTE_KINDS = ("payload", "own half", "duplicate half", "wrapped duplicate", "zero row", "zero run", "inter-orientation pad", "block tail", "tail")
K_PAYLOAD, K_OWN, K_DUP, K_WRAP, K_ZERO_ROW, K_ZERO_RUN, K_ORI_PAD, K_BLOCK_TAIL, K_TAIL = range(len(BYTE_KINDS))
ALLOC_TAIL = 8192   # zero bytes behind the last frame's block of every allocation


def spread_block_index(g):
    """Per byte of one (frame, modality) block of a finer level's spread image: the flat element (row * Wc + column of the matrix of
    R = T * T * Hc rows, i.e. linearize()'s [T * T][cells] array read flat) it holds, -1 where it must be zero, and its kind.
    Flat form: the elements, then zeros.  Banded form: byte k * ls_band_stride + r1 * 32 + c = element (r1 - 1) * Wc + 16 k + c where that
    is an element, for r1 in [0, R + 17): the right halves repeat the next band's left halves, the last band's right half the first 16
    columns of the NEXT row (one band row earlier than the others, hence band row 0), and band rows R + 1 .. R + 16 hold nothing."""
    T, Wc, Hc, n = int(g["T"]), int(g["Wc"]), int(g["Hc"]), int(g["T"]) ** 2 * int(g["cells"])
    idx = np.full(int(g["ls_stride"]), -1, np.int64)
    kind = np.full(int(g["ls_stride"]), K_ZERO_RUN, np.uint8)
    bands = int(g["ls_bands"])
    if not bands:
        idx[:n], kind[:n] = np.arange(n), K_PAYLOAD
        return idx, kind
    rows = T * T * Hc + 17
    assert int(g["ls_band_stride"]) == rows * 32 and bands * 16 == Wc and bands * rows * 32 <= len(idx)
    k, r1, c = np.meshgrid(np.arange(bands), np.arange(rows), np.arange(32), indexing="ij")
    i = (r1 - 1) * Wc + 16 * k + c
    ok = (i >= 0) & (i < n)
    idx[:bands * rows * 32] = np.where(ok, i, -1).reshape(-1)
    kind[:bands * rows * 32] = np.where(~ok, K_ZERO_ROW, np.where(c < 16, K_OWN, np.where(k == bands - 1, K_WRAP, K_DUP))).reshape(-1)
    return idx, kind


def spread_block(g, flat):
    """flat: the oracle's linearize(spread(labels, T), T).  -> (bytes [ls_stride], kinds)."""
    idx, kind = spread_block_index(g)
    flat = np.asarray(flat, np.uint8).reshape(-1)
    assert len(flat) == int(g["T"]) ** 2 * int(g["cells"])
    return np.where(idx >= 0, flat[np.maximum(idx, 0)], 0).astype(np.uint8), kind


def unband_spread_block(g, block):
    """The flat spread image as the debug read takes it out of a block: the first 16 columns of band rows 1 .. R of every band."""
    n = int(g["T"]) ** 2 * int(g["cells"])
    if not g["ls_bands"]:
        return block[:n].copy()
    Wc, bs = int(g["Wc"]), int(g["ls_band_stride"])
    out = np.empty(n, np.uint8)
    for r in range(n // Wc):
        for k in range(int(g["ls_bands"])):
            out[r * Wc + 16 * k:r * Wc + 16 * k + 16] = block[k * bs + (r + 1) * 32:k * bs + (r + 1) * 32 + 16]
    return out


def nibble_block(g, lm):
    """lm: the oracle's linear memories [8][T * T][cells] of the coarsest level (responses 0..4).  Orientation o at o * nib_ori_stride, byte i
    = elem(2 i) | elem(2 i + 1) << 4 for i < (n + 1) / 2, zero everywhere else; the zero run the tables point at starts at nib_zero_off."""
    n = int(g["T"]) ** 2 * int(g["cells"])
    nb, os_, zo = (n + 1) // 2, int(g["nib_ori_stride"]), int(g["nib_zero_off"])
    e = np.zeros((8, 2 * nb), np.uint8)
    e[:, :n] = np.asarray(lm, np.uint8).reshape(8, n)
    out = np.zeros(int(g["nib_mod_stride"]), np.uint8)
    kind = np.full(len(out), K_BLOCK_TAIL, np.uint8)
    kind[:8 * os_] = K_ORI_PAD
    assert nb <= zo and zo + int(g["cells"]) // 2 + 2048 <= os_ and 8 * os_ <= len(out)
    kind[zo:zo + int(g["cells"]) // 2 + 2048] = K_ZERO_RUN
    for o in range(8):
        out[o * os_:o * os_ + nb] = e[o, 0::2] | e[o, 1::2] << 4
        kind[o * os_:o * os_ + nb] = K_PAYLOAD
    return out, kind


def unpack_nibble_block(g, block):
    """-> [8][T * T * cells], as the debug read unpacks it."""
    n = int(g["T"]) ** 2 * int(g["cells"])
    i = np.arange(n)
    return np.stack([block[o * int(g["nib_ori_stride"]) + i // 2] >> 4 * (i % 2) & 15 for o in range(8)]).astype(np.uint8)


def byte_block(g, lm):
    """The byte-wide memories of the generic coarsest-level path: orientation o's T * T * cells bytes at o * ori_stride, zero everywhere else
    (k_pack_nibbles reads up to 15 bytes past each orientation's payload)."""
    n, os_ = int(g["T"]) ** 2 * int(g["cells"]), int(g["ori_stride"])
    out = np.zeros(int(g["mod_stride"]), np.uint8)
    kind = np.full(len(out), K_BLOCK_TAIL, np.uint8)
    kind[:8 * os_] = K_ORI_PAD
    assert int(g["zero_off"]) == n and n <= os_ and 8 * os_ <= len(out)
    kind[n:os_] = K_ZERO_RUN
    for o in range(8):
        out[o * os_:o * os_ + n] = np.asarray(lm, np.uint8).reshape(8, n)[o]
        kind[o * os_:o * os_ + n] = K_PAYLOAD
    return out, kind


def allocation(blocks):
    """[(bytes, kinds)] of an allocation's blocks in order -> (bytes, kinds) of the allocation: the blocks, then ALLOC_TAIL zero bytes."""
    return (np.concatenate([b for b, _ in blocks] + [np.zeros(ALLOC_TAIL, np.uint8)]),
            np.concatenate([k for _, k in blocks] + [np.full(ALLOC_TAIL, K_TAIL, np.uint8)]))


def first_difference(got, want, kind):
    """None where got == want, else (the kind of place of the first differing byte by name, its offset, got, want)."""
    assert got.shape == want.shape == kind.shape, (got.shape, want.shape, kind.shape)
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return BYTE_KINDS[kind[i]], i, int(got[i]), int(want[i])
