"""Seeded cases for the trainer's host half (csrc/lmx_train_select.hpp), shared by tests/test_train_select_host.py (the g++ shim against the
oracle's extractTemplate / cropTemplates) and by the sanitizer program tests/cpp/train_select_main.cpp, which reads them from a file.

A case is a pyramid: {"family", "name", "mods": [modality dicts], "labels": [level][modality] uint8, "mags": [level][modality] float32 or None,
"masks": [level] uint8 or None}.  The single-image families are one-level, one-modality pyramids.  Labels stay in the quantisers' range --
0, a one-hot byte, 255 for normals -- because the oracle's getLabel (like upstream's) has no answer for anything else.  Images are 4x4 up to
64x64.  Densities are chosen so that in every family the oracle accepts at least a third of the cases and rejects at least one
(test_train_select_host.py asserts both)."""
import struct

import numpy as np

STRONG = 55.0
THR_SQ = np.float32(STRONG) * np.float32(STRONG)


def cg(num_features, strong_threshold=STRONG):
    return {"type": "ColorGradient", "num_features": int(num_features), "strong_threshold": float(strong_threshold)}


def dn(num_features, extract_threshold=2):
    return {"type": "DepthNormal", "num_features": int(num_features), "extract_threshold": int(extract_threshold)}


def one_level(family, name, mod, label, mag=None, mask=None):
    return {"family": family, "name": name, "mods": [mod], "labels": [[np.ascontiguousarray(label, np.uint8)]],
            "mags": [[None if mag is None else np.ascontiguousarray(mag, np.float32)]], "masks": None if mask is None else [np.ascontiguousarray(mask, np.uint8)]}


def angles(rng, H, W, density=0.8):
    return ((1 << rng.integers(0, 8, (H, W))) * (rng.random((H, W)) < density)).astype(np.uint8)


def magnitudes(rng, H, W, strong_share=0.7):
    """squared magnitudes: integers (Sobel sums are), `strong_share` of them above the strong threshold"""
    m = rng.integers(3026, 60000, (H, W)).astype(np.float32)
    weak = rng.random((H, W)) >= strong_share
    m[weak] = rng.integers(100, 3026, int(weak.sum())).astype(np.float32)
    return m


def blocks(rng, H, W, b, p255=0.03, p0=0.05):
    """block-constant normal labels (distances to another label exceed 1), some 255 and 0 pixels"""
    a = (1 << rng.integers(0, 8, (H // b + 1, W // b + 1))).astype(np.uint8)
    a = np.kron(a, np.ones((b, b), np.uint8))[:H, :W].copy()
    r = rng.random((H, W))
    a[r < p255] = 255
    a[(r >= p255) & (r < p255 + p0)] = 0
    return a


def mask_variants(rng, H, W):
    """-> list of (name, mask or None)"""
    def box(y0, y1, x0, x1, v=255):
        m = np.zeros((H, W), np.uint8)
        m[max(0, y0):y1, max(0, x0):x1] = v
        return m
    h2, w2 = max(2, H // 2), max(2, W // 2)
    out = [("none", None), ("zero", np.zeros((H, W), np.uint8)), ("whole", np.full((H, W), 255, np.uint8)),
           ("left", box(H // 4, H - H // 4, 0, w2)), ("right", box(H // 4, H - H // 4, W - w2, W)),
           ("top", box(0, h2, W // 4, W - W // 4)), ("bottom", box(H - h2, H, W // 4, W - W // 4)),
           ("corner_tl", box(0, h2, 0, w2)), ("corner_tr", box(0, h2, W - w2, W)), ("corner_bl", box(H - h2, H, 0, w2)), ("corner_br", box(H - h2, H, W - w2, W)),
           ("near_1", box(1, H - 1, 1, W - 1)), ("near_2", box(2, H - 2, 2, W - 2)), ("near_tl_1_2", box(1, h2 + 2, 2, w2 + 2)),
           ("column", box(0, H, W // 2, W // 2 + 1)), ("row", box(H // 2, H // 2 + 1, 0, W)),
           ("two_blobs", box(0, H // 2 - 1, 0, W // 2 - 1) | box(H // 2 + 1, H, W // 2 + 1, W)),
           ("value_1", box(H // 5, H - H // 5, W // 5, W - W // 5, 1)), ("value_128", box(H // 5, H - H // 5, W // 5, W - W // 5, 128)),
           ("random_values", (box(1, H - 1, 1, W - 1) > 0) * rng.integers(1, 256, (H, W)).astype(np.uint8))]
    dots = np.zeros((H, W), np.uint8)
    dots[1::2, 1::2] = 255          # only odd coordinates: the next level's mask is empty
    out.append(("odd_dots", dots))
    return out


def family_masks(kind):
    """every mask variant at several sizes, on dense label images"""
    rng = np.random.default_rng([11, kind == "color"])
    out = []
    for H, W in ((4, 4), (9, 7), (16, 16), (23, 40), (41, 33), (64, 64), (64, 37)):
        for name, mask in mask_variants(rng, H, W):
            nf = int(rng.choice([1, 2, 3, 5, 9, 20]))
            if kind == "color":
                out.append(one_level("masks_color", "%s_%dx%d" % (name, W, H), cg(nf), angles(rng, H, W, 0.9), magnitudes(rng, H, W, 0.85), mask))
            else:
                out.append(one_level("masks_depth", "%s_%dx%d" % (name, W, H), dn(nf, int(rng.integers(0, 3))), blocks(rng, H, W, int(rng.integers(3, 9))), None, mask))
    return out


def family_color_ties():
    """few distinct magnitudes: the stable sort keeps raster order inside a tie"""
    rng = np.random.default_rng(12)
    out = []
    for i in range(24):
        H, W = (int(v) for v in rng.integers(5, 50, 2))
        mag = rng.choice(np.asarray([3000.0, 3026.0, 4000.0, 4001.0, 50000.0], np.float32), (H, W))
        mask = None if i % 3 == 0 else mask_variants(rng, H, W)[int(rng.integers(2, 20))][1]
        out.append(one_level("color_ties", "ties_%d" % i, cg(int(rng.choice([1, 2, 4, 8, 31, 63]))), angles(rng, H, W), mag, mask))
    return out


def family_color_threshold():
    """magnitudes exactly strong_threshold^2 and one ulp either side: only the upper neighbour is a candidate"""
    rng = np.random.default_rng(13)
    lo, hi = np.nextafter(THR_SQ, np.float32(0)), np.nextafter(THR_SQ, np.float32(1e9))
    out = []
    for i in range(18):
        H, W = (int(v) for v in rng.integers(4, 30, 2))
        mag = rng.choice(np.asarray([lo, THR_SQ, hi], np.float32), (H, W))
        n_hi = int(((mag == hi)).sum())
        ang = np.where(angles(rng, H, W, 1.0) == 0, 1, angles(rng, H, W, 1.0)).astype(np.uint8)
        nf = max(1, min(63, n_hi + (1 if i % 3 == 0 else -int(rng.integers(0, 5)))))     # a third one above the count: rejected
        out.append(one_level("color_threshold", "thr_%d" % i, cg(nf), ang, mag, None))
    return out


def family_color_counts():
    """candidates == num_features, num_features - 1 and 50 x num_features (a large first distance, many restarts), num_features 1, 2, 31, 63"""
    rng = np.random.default_rng(14)
    out = []
    for nf in (1, 2, 31, 63):
        for what, count in (("equal", nf), ("one_less", nf - 1), ("x50", 50 * nf), ("x50_clustered", 50 * nf)):
            H = W = 64 if count > 1000 else 40
            ang, mag = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32)
            if what == "x50_clustered":      # all candidates in a compact block: the first distance fits nothing but the first few
                side = int(np.ceil(np.sqrt(count)))
                idx = (np.arange(count) // side + 3) * W + np.arange(count) % side + 2
            else:
                idx = rng.choice(H * W, count, replace=False)
            ang.reshape(-1)[idx] = 1 << rng.integers(0, 8, count)
            mag.reshape(-1)[idx] = rng.integers(3026, 9000, count).astype(np.float32)
            out.append(one_level("color_counts", "%s_%d" % (what, nf), cg(nf), ang, mag, None))
    return out


def family_depth_blocks():
    """block-constant labels, 255 pixels, extract_threshold 0 .. 3"""
    rng = np.random.default_rng(15)
    out = []
    for i in range(40):
        H, W = (int(v) for v in rng.integers(6, 65, 2))
        mask = None if i % 2 == 0 else mask_variants(rng, H, W)[int(rng.integers(2, 20))][1]
        out.append(one_level("depth_blocks", "blocks_%d" % i, dn(int(rng.choice([1, 2, 3, 6, 12, 31, 63])), i % 4), blocks(rng, H, W, int(rng.integers(2, 10)), p255=0.05 * (i % 3)), None, mask))
    return out


def family_depth_label_ties():
    """one label holding every candidate against eight labels with equal counts: the scores divided by the label count tie across labels"""
    out = []
    for H, W in ((16, 16), (24, 32), (33, 47), (64, 64)):
        for et in (0, 1, 2, 3):
            for nf in (1, 4, 63):
                one = np.full((H, W), 1 << (et + nf) % 8, np.uint8)
                one[0, :] = 0                                              # zero pixels, so that the distances are finite
                out.append(one_level("depth_label_ties", "one_label_%dx%d_%d_%d" % (W, H, et, nf), dn(nf, et), one, None, None))
                bw = W // 8                                                # eight vertical stripes of equal width, the rest 0
                eight = np.zeros((H, W), np.uint8)
                for k in range(8):
                    eight[:, k * bw:(k + 1) * bw] = 1 << k
                out.append(one_level("depth_label_ties", "eight_labels_%dx%d_%d_%d" % (W, H, et, nf), dn(nf, et), eight, None, None))
    return out


def down(a):
    return np.ascontiguousarray(a[::2, ::2][:a.shape[0] // 2, :a.shape[1] // 2])


def family_pyramids():
    """two and three levels, both modalities, odd widths and heights at every level; masks from the variants (odd_dots: level 0 accepts,
    level 1 has an empty mask and rejects)"""
    rng = np.random.default_rng(16)
    out = []
    sizes = [(63, 47), (47, 63), (55, 31), (31, 55), (63, 63), (64, 48)]
    for i in range(36):
        L = 2 + i % 2
        W, H = sizes[i % len(sizes)]
        variants = mask_variants(rng, H, W)
        name, mask = variants[i % len(variants)] if i % 4 else ("odd_dots", variants[-1][1])
        nf = int(rng.choice([4, 8, 12])) if name != "odd_dots" else 4
        # isolated dots do not survive DepthNormal's two erosions even at level 0: those cases are ColorGradient alone
        mods = [cg(nf), dn(nf, int(rng.integers(0, 4)))][:1 if name == "odd_dots" else 2]
        labels, mags, masks = [], [], []
        normal = blocks(rng, H, W, int(rng.integers(4, 10)))
        for l in range(L):
            h, w = H >> l, W >> l
            labels.append([angles(rng, h, w, 0.95), normal][:len(mods)])
            mags.append([magnitudes(rng, h, w, 0.9), None][:len(mods)])
            masks.append(mask)
            normal = down(normal)
            mask = None if mask is None else down(mask)
        out.append({"family": "pyramids", "name": "L%d_%dx%d_%s_%d" % (L, W, H, name, i), "mods": mods, "labels": labels, "mags": mags,
                    "masks": None if masks[0] is None else masks})
    # a 12x12 box: level 0 has 64 pixels inside the twice-eroded mask, level 1 (6x6) has 4 < 12 / 2 -- DepthNormal rejects at level 1 only
    for i, (W, H) in enumerate(sizes[:3]):
        mask = np.zeros((H, W), np.uint8)
        mask[10 + i:22 + i, 14 - i:26 - i] = 255
        normal = np.full((H, W), 1 << i, np.uint8)
        labels = [[angles(rng, H >> l, W >> l, 1.0), down(normal) if l else normal] for l in range(2)]
        mags = [[np.full((H >> l, W >> l), 9000.0, np.float32), None] for l in range(2)]
        out.append({"family": "pyramids", "name": "L2_%dx%d_box12_level1_only_%d" % (W, H, i), "mods": [cg(12), dn(12, 0)], "labels": labels, "mags": mags,
                    "masks": [mask, down(mask)]})
    return out


def family_zero_features():
    """a level whose num_features is (halved to) 0: refused before any division; no oracle answer exists (upstream divides by zero)"""
    rng = np.random.default_rng(17)
    out = []
    for mods, L in (([cg(0)], 1), ([dn(0)], 1), ([cg(1)], 2), ([dn(1, 2)], 2), ([cg(3)], 3), ([cg(8), dn(1)], 2), ([cg(-4)], 1)):
        labels, mags = [], []
        for l in range(L):
            h, w = 32 >> l, 40 >> l
            labels.append([angles(rng, h, w, 0.9) if m["type"] == "ColorGradient" else blocks(rng, h, w, 4) for m in mods])
            mags.append([magnitudes(rng, h, w, 0.9) if m["type"] == "ColorGradient" else None for m in mods])
        out.append({"family": "zero_features", "name": "L%d_%s" % (L, "_".join("%s%d" % (m["type"][0], m["num_features"]) for m in mods)), "mods": mods,
                    "labels": labels, "mags": mags, "masks": None})
    return out


def all_cases():
    return (family_masks("color") + family_masks("depth") + family_color_ties() + family_color_threshold() + family_color_counts() + family_depth_blocks() +
            family_depth_label_ties() + family_pyramids())


def write_cases(path, cases):
    """the file tests/cpp/train_select_main.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            L, M = len(c["labels"]), len(c["mods"])
            f.write(struct.pack("<ii", L, M))
            for m in c["mods"]:
                f.write(struct.pack("<iifi", m["type"] == "ColorGradient", m["num_features"], m.get("strong_threshold", STRONG), m.get("extract_threshold", 2)))
            for l in range(L):
                h, w = c["labels"][l][0].shape
                f.write(struct.pack("<iii", h, w, c["masks"] is not None))
                for k in range(M):
                    f.write(np.ascontiguousarray(c["labels"][l][k], np.uint8).tobytes())
                    if c["mods"][k]["type"] == "ColorGradient":
                        f.write(np.ascontiguousarray(c["mags"][l][k], "<f4").tobytes())
                if c["masks"] is not None:
                    f.write(np.ascontiguousarray(c["masks"][l], np.uint8).tobytes())
