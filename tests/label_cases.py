"""Built label images for the stages behind the quantisers: spread / linearise, coarse scoring, refinement.

Pure numpy, no device.  Every family hands back Cases: a hand-built TemplateBank (template rows (w, h, level, first, count) and features
(x, y, label) written out by `make_bank`), frames of label images [level][modality] -> uint8 (H_l, W_l), the threshold(s) of the call, and the
CLAIMS the case exists for -- "placement 7 of template 2 has raw == raw_threshold" -- as data.  tests/test_label_cases_host.py checks every
claim against the reference (the oracle's spread -> response maps -> linear memories -> similarity -> similarityLocal) and against mutants of
the numpy restatement; tests/test_gpu_label_match.py sends the same cases through Detector.debug_enqueue_labels.

Labels are one-hot, as the quantisers write them.  A spread byte with several bits is the OR of several one-hot pixels inside one T x T
window.  Orientation distance 0..4 between a pixel's bit and a feature's label gives response 4..0 (for bits 4..7 the distance is not
circular: SIMILARITY_LUT's asymmetry), so the planter picks, per feature and wanted response, a bit from the table itself.

Geometry of an instance.  A template's features of one (level, modality) sit at (cell * T + phase) with ONE phase for all of them and distinct
cells: two features are then at least T apart, no planted pixel lies in another feature's T x T window, and the sum at the planted placement
is exactly the sum of the wanted responses.  (Other placements see strays; what they add up to is the reference's business.)  Where only
full responses are wanted the features may share a cell: each still sees its own pixel."""
import functools
from types import SimpleNamespace

import numpy as np

import np_restatement as R
from linemod_pose_estimation_amd import synth
from linemod_pose_estimation_amd.bank import TemplateBank

F32 = np.float32
CG, DN = "ColorGradient", "DepthNormal"
LUT = R.similarity_lut_from_rule()
# RESP[o][b]: response of a feature with label o to the one-hot pixel 1 << b
RESP = np.array([[max(LUT[32 * o + ((1 << b) & 15)], LUT[32 * o + 16 + ((1 << b) >> 4)]) for b in range(8)] for o in range(8)], np.int64)


def response_of(o, v):
    """Response of orientation o to spread byte v, from the rule."""
    return int(max(LUT[32 * o + (v & 15)], LUT[32 * o + 16 + (v >> 4)]))


def bit_for(label, r):
    """A bit whose one-hot pixel gives a feature of `label` the response r (1..4)."""
    hits = np.flatnonzero(RESP[label] == r)
    assert len(hits), (label, r)
    return int(hits[0])


def modality(kind):
    return dict(synth.DEFAULT_COLOR_GRADIENT if kind == CG else synth.DEFAULT_DEPTH_NORMAL)


def make_bank(T, mods, classes):
    """classes: {class id: [template]}, template = [level][modality] -> (w, h, [(x, y, label), ...]).  Rows and features are written out in the
    wire order: template, level, modality."""
    bank = TemplateBank(T=list(T), modalities=[modality(k) for k in mods])
    L, M = len(T), len(mods)
    for cid in classes:
        rows, feats = [], []
        for tpl in classes[cid]:
            assert len(tpl) == L and all(len(lv) == M for lv in tpl)
            for l in range(L):
                for m in range(M):
                    w, h, f = tpl[l][m]
                    rows.append((w, h, l, len(feats), len(f)))
                    feats += [tuple(int(v) for v in x) for x in f]
        bank.classes.append((cid, np.asarray(rows, np.int32).reshape(-1, 5), np.asarray(feats, np.int32).reshape(-1, 3)))
    return bank


def template_of(bank, cid, tid):
    """-> [level][modality] -> (w, h, features int array [n, 3])."""
    L, M = len(bank.T), len(bank.modalities)
    t = bank.get_templates(cid, tid)
    return [[(t[l * M + m][0], t[l * M + m][1], t[l * M + m][3]) for m in range(M)] for l in range(L)]


def blank(bank, W, H):
    return [[np.zeros((H >> l, W >> l), np.uint8) for _ in bank.modalities] for l in range(len(bank.T))]


def put(img, x, y, bit):
    """One one-hot pixel; a pixel that is already set must hold the same bit (the planter never needs two bits in one pixel)."""
    assert 0 <= x < img.shape[1] and 0 <= y < img.shape[0], (x, y, img.shape)
    assert img[y, x] in (0, 1 << bit), (x, y, int(img[y, x]), bit)
    img[y, x] = 1 << bit


def plant(img, T, cell_xy, feats, responses=None):
    """Feature i of `feats` placed at cell (cx, cy) of a level with cell size T sees response responses[i] (default 4): its pixel goes to
    the first pixel of its window, (cx * T + x, cy * T + y)."""
    cx, cy = cell_xy
    for i, (x, y, lab) in enumerate(np.asarray(feats).reshape(-1, 3).tolist()):
        r = 4 if responses is None else int(responses[i])
        if r > 0:
            put(img, cx * T + x, cy * T + y, bit_for(lab, r))


def offset_of(T):
    return T // 2 + (T % 2 - 1)


def patch_origin(bank, W, H, tpl, level, x, y):
    """The refinement step into `level` of a candidate at (x, y) of level + 1: -> (ocx, ocy), the patch's first cell (may be negative)."""
    T = bank.T[level]
    w, h = W >> level, H >> level
    border = 8 * T
    x, y = 2 * x + 1, 2 * y + 1
    x, y = max(x, border), max(y, border)
    x, y = min(x, w - tpl[level][0][0] - border), min(y, h - tpl[level][0][1] - border)
    return int(x / T) - 8, int(y / T) - 8


def plant_linear(img, T, placement, feats):
    """A full-response instance at a coarsest-level PLACEMENT, the way similarity() addresses it: feature (x, y) reads element placement +
    (y // T) * Wc + x // T of its phase's linear memory, which for placements near the end of a row of cells lies in the next row."""
    Wc = img.shape[1] // T
    for x, y, lab in np.asarray(feats).reshape(-1, 3).tolist():
        cell = placement + (y // T) * Wc + x // T
        put(img, cell % Wc * T + x % T, cell // Wc * T + y % T, bit_for(lab, 4))


def plant_pyramid(labels, bank, W, H, tpl, coarse_cell, patch_cell=(8, 8), responses=None, linear=False):
    """A full-response instance of `tpl` at `coarse_cell` of the coarsest level and, level by level, at cell `patch_cell` of the patch the
    refinement opens there.  responses: {(level, modality): list} lowers single responses.  -> the match position the chain ends at."""
    L, M = len(bank.T), len(bank.modalities)
    responses = responses or {}
    cx, cy = coarse_cell
    for m in range(M):
        if linear:
            plant_linear(labels[L - 1][m], bank.T[L - 1], cy * (labels[L - 1][m].shape[1] // bank.T[L - 1]) + cx, tpl[L - 1][m][2])
        else:
            plant(labels[L - 1][m], bank.T[L - 1], (cx, cy), tpl[L - 1][m][2], responses.get((L - 1, m)))
    x, y = cx * bank.T[L - 1] + offset_of(bank.T[L - 1]), cy * bank.T[L - 1] + offset_of(bank.T[L - 1])
    for l in range(L - 2, -1, -1):
        ocx, ocy = patch_origin(bank, W, H, tpl, l, x, y)
        px, py = ocx + patch_cell[0], ocy + patch_cell[1]
        for m in range(M):
            plant(labels[l][m], bank.T[l], (px, py), tpl[l][m][2], responses.get((l, m)))
        x, y = px * bank.T[l] + offset_of(bank.T[l]), py * bank.T[l] + offset_of(bank.T[l])
    return x, y


def grid_features(n, T, phase, labels, cols=8, cell0=(0, 0)):
    """n features at distinct cells (row-major over `cols` columns from cell0), all with one phase; labels cycles."""
    return [((cell0[0] + i % cols) * T + phase[0], (cell0[1] + i // cols) * T + phase[1], labels[i % len(labels)]) for i in range(n)]


def extent(feats, T):
    """Declared (w, h) that spans the features' cells exactly."""
    f = np.asarray(feats).reshape(-1, 3)
    if not len(f):
        return T, T
    return (int(f[:, 0].max()) // T + 1) * T, (int(f[:, 1].max()) // T + 1) * T


def full_tile(img, T, cells=None):
    """One-hot pixels with pixel (x, y) -> bit (x % T + (y % T) * T) % 8: every T x T window holds all eight bits, every spread byte is
    0xff.  cells: boolean [Hc, Wc] selects whole cells (their windows at the cell anchor are 0xff), default all."""
    H, W = img.shape
    y, x = np.mgrid[0:H, 0:W]
    tile = (1 << ((x % T + (y % T) * T) % 8)).astype(np.uint8)
    assert T * T >= 8
    if cells is None:
        img[:] = tile
    else:
        sel = np.kron(cells.astype(np.uint8), np.ones((T, T), np.uint8)).astype(bool)
        img[sel] = tile[sel]


def byte_in_cell(img, T, cell_xy, v):
    """Spread byte v at the anchor of a cell: bit b of v as a one-hot pixel at pixel b (row-major) of the cell's T x T block."""
    cx, cy = cell_xy
    for b in range(8):
        if v >> b & 1:
            put(img, cx * T + b % T, cy * T + b // T, b)


def Case(name, bank, W, H, frames, threshold, class_ids=(), claims=None, **kw):
    return SimpleNamespace(name=name, bank=bank, W=W, H=H, frames=frames, threshold=threshold, class_ids=tuple(class_ids), claims=claims or [],
                           max_candidates=kw.pop("max_candidates", 1 << 16), **kw)


def stack(case, idx=None):
    """The frames `idx` of a case as Detector.debug_enqueue_labels takes them: [level][modality] -> [n, H_l, W_l]."""
    idx = range(len(case.frames)) if idx is None else idx
    L, M = len(case.bank.T), len(case.bank.modalities)
    return [[np.stack([case.frames[f][l][m] for f in idx]) for m in range(M)] for l in range(L)]


# ---- R: the response tables ------------------------------------------------------------------------------------------------------------
R_COARSE_GEOMS = {   # the three classes of the coarsest level's spread (tests/test_gpu_buffer_bytes.py)
    "fused_nibbles": ((4, 8), 256, 192),        # k_small_spread<4, 8> for one and two frames, nibbles written directly
    "bytes_then_pack": ((5, 8), 320, 240),      # byte-wide memories, k_pack_nibbles
    "generic_odd_width": ((5, 8), 240, 160),    # level 1 is 120 x 80, Wc = 15: the generic kernel, Wc % 8 != 0
}


def r_coarse(geom):
    """All 256 spread bytes at cell anchors of the coarsest level, each at every (cell index mod 8) of the nibble packing.  Cell idx of
    frame f holds byte (idx // 8 + f * (cells // 8)) % 256; level 0 carries a sparse random one-hot image."""
    T, W, H = R_COARSE_GEOMS[geom]
    one = [[(T[l], T[l], [(0, 0, 0)])] for l in range(2)]
    bank = make_bank(T, (CG,), {"r": [one]})
    Wc, Hc = (W >> 1) // T[1], (H >> 1) // T[1]
    per = Wc * Hc // 8
    n_frames = -(-256 // per)
    rng = np.random.default_rng(7)
    frames = []
    for f in range(n_frames):
        lab = blank(bank, W, H)
        for idx in range(Wc * Hc):
            byte_in_cell(lab[1][0], T[1], (idx % Wc, idx // Wc), (idx // 8 + f * per) % 256)
        lab[0][0][:] = np.where(rng.uniform(0, 1, (H, W)) < 0.2, 1 << rng.integers(0, 8, (H, W)), 0).astype(np.uint8)
        frames.append(lab)
    claims = [dict(kind="coarse_bytes", level=1, Wc=Wc, Hc=Hc, T=T[1])]
    return Case("r_coarse_" + geom, bank, W, H, frames, 50.0, claims=claims, linear_memories=True)


R_FINE_W, R_FINE_H, R_FINE_T = 320, 240, (5, 8)
NEIGHBOURS = ("0x00", "0x7f", "0x80", "0xfe_without_target")


def neighbour_byte(kind, v):
    return {"0x00": 0, "0x7f": 0x7f, "0x80": 0x80, "0xfe_without_target": 0xfe & ~v}[kind]


def r_fine_expectations(variant):
    """The (orientation, target byte, neighbour kind, response) the variant is for: the template of that orientation has a match of
    similarity 25 x response at the target's window (none for response 0).  plain: all 8 x 256.  neighbours: the triples whose neighbour
    byte answers strictly less than a target that answers at all -- there the target is the patch's only best cell whatever the three
    cells sharing its dword add; a neighbour that answers as well as its target (0x7f for orientations 0..6, 0x80 for orientation 7, and
    0xfe-without-the-target for many) leaves the reference's result to the first maximum, which the comparison with the oracle covers."""
    if variant == "plain":
        return [(o, v, None, response_of(o, v)) for v in range(256) for o in range(8)]
    return [(o, v, k, response_of(o, v)) for k in NEIGHBOURS for v in range(256) for o in range(8)
            if response_of(o, v) > response_of(o, neighbour_byte(k, v))]


def r_fine(variant):
    """Eight one-feature templates, one per orientation, feature (0, 0) at both levels.  Level 0: `windows` -- cells whose 5 x 5 block ORs to a
    chosen byte -- at cells (8 + 16 i, 8 + 16 j), so that every 16 x 16 patch holds exactly one window column and row; a candidate's best cell
    is its window, its similarity 25 x response4(window byte).  variant "plain": all 256 bytes, every coarse placement a candidate (level 1 is
    0xff everywhere).  variant "neighbours": the three cells on either side of the window (whichever three share the lane's dword with it)
    carry 0x00 / 0x7f / 0x80 / 0xfe without the target's bits, for all 256 targets; candidates in one row of coarse cells per window row."""
    T, W, H = R_FINE_T, R_FINE_W, R_FINE_H
    bank = make_bank(T, (CG,), {"r": [[[(T[l], T[l], [(0, 0, o)])] for l in range(2)] for o in range(8)]})
    wins = [(8 + 16 * i, 8 + 16 * j) for j in range(3) for i in range(4)]
    todo = [(v, None) for v in range(256)] if variant == "plain" else [(v, k) for k in NEIGHBOURS for v in range(256)]
    frames, where = [], []
    for f0 in range(0, len(todo), len(wins)):
        lab = blank(bank, W, H)
        if variant == "plain":
            full_tile(lab[1][0], T[1])
        else:
            cells = np.zeros(((H >> 1) // T[1], (W >> 1) // T[1]), bool)
            cells[[2, 7, 12], :] = True      # coarse rows 2, 7, 12 open patches over window rows 8, 24, 40
            full_tile(lab[1][0], T[1], cells)
        for (v, k), (cx, cy) in zip(todo[f0:f0 + len(wins)], wins):
            byte_in_cell(lab[0][0], T[0], (cx, cy), v)
            if k is not None:
                for d in (-3, -2, -1, 1, 2, 3):
                    byte_in_cell(lab[0][0], T[0], (cx + d, cy), neighbour_byte(k, v))
            where.append((len(frames), cx, cy, v, k))
        frames.append(lab)
    claims = [dict(kind="fine_windows", where=where, variant=variant, expect=r_fine_expectations(variant))]
    return Case("r_fine_" + variant, bank, W, H, frames, 20.0, claims=claims)


R_FINE3_T, R_FINE3_SIZE, R_FINE3_THRESHOLDS = (4, 8, 10), 320, (20.0, 45.0, 70.0, 90.0)


def r_fine_levels3():
    """L = 3: the byte sits at level 1 (one window per frame, at cell (8, 8) of the 20 x 20: every level-1 patch holds it), level 2 opens a few
    candidates per template and level 0 answers 4 everywhere.  A candidate survives level 1 when 25 x response4(byte) >= threshold, so the four
    thresholds read the response out; the coarsest level has four features per template so that its own test passes up to 90."""
    T, S = R_FINE3_T, R_FINE3_SIZE
    coarse = lambda o: [(1, 2, o), (6, 3, o), (3, 7, o), (8, 8, o)]
    bank = make_bank(T, (CG,), {"r": [[[(T[0], T[0], [(0, 0, o)])], [(T[1], T[1], [(0, 0, o)])], [(T[2], T[2], coarse(o))]] for o in range(8)]})
    cells = np.zeros((8, 8), bool)
    cells[2:5, 2:5] = True      # the features' windows reach one cell to the right and below: placements (2..3, 2..3) see 0xff four times
    frames = []
    for v in range(256):
        lab = blank(bank, S, S)
        full_tile(lab[2][0], T[2], cells)
        byte_in_cell(lab[1][0], T[1], (8, 8), v)
        full_tile(lab[0][0], T[0])
        frames.append(lab)
    # level 1 ends at cell (8, 8): (67, 67); level 0 opens its patch at cell 135 // 4 - 8 = 25 and its first cell wins
    xy = (25 * T[0] + offset_of(T[0]), 25 * T[0] + offset_of(T[0]))
    return [Case("r_fine_levels3_thr%g" % thr, bank, S, S, frames, thr, claims=[dict(kind="fine_level1", xy=xy)]) for thr in R_FINE3_THRESHOLDS]


# ---- S: sums, thresholds, the pruning bound ---------------------------------------------------------------------------------------------
S_W, S_H, S_T = 320, 240, (5, 8)
S_COUNTS = (1, 2, 3, 4, 12, 13, 15, 16, 17, 30, 31, 45, 46, 62, 63)
S_COUNTS_WIDE = (64, 95, 126)       # two modalities, beyond the block table: generic and u8 only; 126 = 63 + 63
S_THRESHOLDS = (50.0, 75.0, 80.0, 92.0, 99.9)
S_PLACEMENTS = ((1, 2), (11, 4))    # cells of the instance with raw == raw_threshold and of the one with raw_threshold + 1: 8 x 8-cell blocks apart


def s_template(nf_per_mod, seed):
    """Coarsest level: nf features per modality on an 8-column grid of cells with one phase; level 0: three features in one cell."""
    rng = np.random.default_rng(seed)
    lv1, lv0 = [], []
    for m, nf in enumerate(nf_per_mod):
        f1 = grid_features(nf, S_T[1], (int(rng.integers(0, 8)), int(rng.integers(0, 8))), rng.integers(0, 8, 8).tolist())
        lv1.append((64, 64, f1))
        lv0.append((128, 128, [(1, 1, (m + 1) % 8), (3, 2, (m + 4) % 8), (2, 4, (m + 6) % 8)]))
    return [lv0, lv1]


def split(nf, M):
    return (nf,) if M == 1 else (nf - nf // 2, nf // 2)


@functools.lru_cache(maxsize=None)
def s_bank(M, counts=S_COUNTS):
    mods = (CG, DN)[:M]
    return make_bank(S_T, mods, {"s": [s_template(split(nf, M), 100 * M + nf) for nf in counts]})


def lowered(nf_per_mod, total, order):
    """Responses (per modality) that sum to `total`: every feature 4, then the deficit is taken from the features in `order` (a list of
    (modality, feature index)), 4 at a time."""
    resp = [[4] * n for n in nf_per_mod]
    deficit = 4 * sum(nf_per_mod) - total
    assert deficit >= 0
    for m, i in order:
        take = min(4, deficit)
        resp[m][i] -= take
        deficit -= take
        if deficit == 0:
            break
    assert deficit == 0
    return resp


def s_thresholds(M, counts=S_COUNTS, name="s", table_order=None, thresholds=S_THRESHOLDS):
    """Per threshold one call of len(counts) frames: frame k holds two instances of template k, one with raw == raw_threshold (no candidate)
    and one with raw_threshold + 1 (a candidate) where 4 nf allows it.  Which responses are lowered: `table_order` None -> spread evenly
    from the last feature backwards; else {template: [(modality, feature)] in the kernel's table order} and the pattern of the frame
    -- missing part first (every later bound test sees S == need), missing part last, a random subset."""
    bank = s_bank(M, counts)
    cases = []
    for thr in thresholds:
        for pattern in (("even",) if table_order is None else ("first", "last", "random")):
            frames, claims = [], []
            for k, nf in enumerate(counts):
                tpl = template_of(bank, "s", k)
                per_mod = [len(tpl[1][m][2]) for m in range(M)]
                rt = R.raw_threshold(nf, thr)
                lab = blank(bank, S_W, S_H)
                feats = [(m, i) for m in range(M) for i in range(per_mod[m])]
                if table_order is None:
                    order = feats[::-1]
                else:
                    order = {"first": table_order[k], "last": table_order[k][::-1],
                             "random": [table_order[k][j] for j in np.random.default_rng(int(thr * 10) + k).permutation(len(feats))]}[pattern]
                for cell, total in zip(S_PLACEMENTS, (rt, rt + 1)):
                    if total > 4 * nf:
                        continue    # raw_threshold == 4 nf: no sum can exceed it, the template has no candidate at this threshold
                    resp = lowered(per_mod, total, order)
                    plant_pyramid(lab, bank, S_W, S_H, tpl, cell, responses={(1, m): resp[m] for m in range(M)})
                    claims.append(dict(kind="coarse_sum", frame=k, template=k, cell=cell, total=total, raw_threshold=rt, candidate=total > rt,
                                       tight=pattern == "first" and total == rt + 1))
                frames.append(lab)
            cases.append(Case("%s_M%d_thr%s_%s" % (name, M, thr, pattern), bank, S_W, S_H, frames, thr, claims=claims))
    return cases


def saturated(M, W=640, H=480, n_templates=8):
    """A constant label image (bit 0 everywhere, both levels, every modality) and templates whose 63 features per modality all have label 0:
    every response is 4, every byte sum 252, every placement of every template a candidate and a match of similarity 100."""
    mods = (CG, DN, CG)[:M]
    tpls = []
    for t in range(n_templates):
        lv = []
        for l in range(2):
            f = grid_features(63, S_T[l], (t % S_T[l], (3 * t) % S_T[l]), [0], cols=7 + t % 3)
            lv.append([(extent(f, S_T[l])[0], extent(f, S_T[l])[1], f)] * M)
        tpls.append(lv)
    bank = make_bank(S_T, mods, {"sat": tpls})
    lab = blank(bank, W, H)
    for l in range(2):
        for m in range(M):
            lab[l][m][:] = 1
    return Case("saturated_M%d_%dx%d" % (M, W, H), bank, W, H, [lab, lab], 90.0, claims=[dict(kind="saturated", M=M)], max_candidates=1 << 15)


def per_class_edges():
    """Two classes, each with its own threshold and an instance on either side of ITS equality edge, and a third class that is not matched."""
    nfs = {"a": 17, "b": 46, "c": 30}
    thr = {"a": 75.0, "b": 92.0}
    bank = make_bank(S_T, (CG, DN), {c: [s_template(split(nf, 2), 900 + nf)] for c, nf in nfs.items()})
    frames, claims = [], []
    for k, c in enumerate(sorted(nfs)):
        tpl = template_of(bank, c, 0)
        per_mod = [len(tpl[1][m][2]) for m in range(2)]
        rt = R.raw_threshold(nfs[c], thr.get(c, 75.0))
        lab = blank(bank, S_W, S_H)
        order = [(m, i) for m in range(2) for i in range(per_mod[m])][::-1]
        for cell, total in zip(S_PLACEMENTS, (rt, rt + 1)):
            resp = lowered(per_mod, total, order)
            plant_pyramid(lab, bank, S_W, S_H, tpl, cell, responses={(1, m): resp[m] for m in range(2)})
            if c in thr:
                claims.append(dict(kind="coarse_sum", frame=k, template=0, cls=c, cell=cell, total=total, raw_threshold=rt, candidate=total > rt, tight=False))
        frames.append(lab)
    return Case("per_class_edges", bank, S_W, S_H, frames, thr, claims=claims)


# ---- P: positions ------------------------------------------------------------------------------------------------------------------------
CHUNK_POS = 504
P_FRAME_COUNTS = (1, 2, 7, 8, 9, 16, 17)


@functools.lru_cache(maxsize=None)
def p_bank(T, W, H):
    """t0: eight features in eight cells of one row (all eight nibble shifts of a lane's dword), one cell high: as many placements as the
    grid allows.  t1: the same features under a declared extent of 32 x 5 cells, which leaves a tail of a single placement behind the
    two-chunk pass at 640x480 (tests/test_gpu_score_tail.py: WIDE)."""
    T1 = T[1]
    f1 = [(i * T1 + (3 * i + 1) % T1, (5 * i + 2) % T1, (i * 3) % 8) for i in range(8)]
    f0 = [(1, 1, 2), (3, 0, 5), (0, 3, 7)]
    t0 = [[(2 * T1 * 8, 2 * T1, f0)], [(T1 * 8, T1, f1)]]
    t1 = [[(498, 2 * T1 * 5, f0)], [(249, T1 * 5, f1)]]
    return make_bank(T, (CG,), {"p": [t0, t1]})


def p_targets(T, W, H):
    """-> {template: [placement]}"""
    Wc, Hc = (W >> 1) // T[1], (H >> 1) // T[1]
    pos0 = (Hc - 1) * Wc + (Wc - 8) + 1
    pos1 = (Hc - 5) * Wc + (Wc - 32) + 1
    tail0 = (pos0 - 1) // (2 * CHUNK_POS) * (2 * CHUNK_POS)
    t0 = [0, 7, 8, 503, 504, 1007, 1008, pos0 - 1]
    t0 += [tail0 + 8 * d for d in (30, 31, 32) if tail0 + 8 * d + 7 < pos0]     # tail dwords 30, 31, 32 where the tail has them
    t0 += [tail0 + 8 * d + 7 for d in (30, 31, 32) if tail0 + 8 * d + 7 < pos0]
    t0.append((pos0 - 1) // 8 * 8)                                                # first placement of the last live dword
    t1 = [p for p in (0, 503, 504, 1007, 1008, pos1 - 1) if p < pos1]
    return {0: sorted(set(t0)), 1: sorted(set(t1))}, (pos0, pos1), (Wc, Hc)


def positions(T, W, H, n_frames, second):
    """One call of n_frames: the frame with the instances is the first of a wave's pair (frame 0) or the second (frame 8, n_frames > 8),
    every other frame is all zero.  Every target placement of both templates carries a full-response instance."""
    bank = p_bank(T, W, H)
    targets, npos, (Wc, Hc) = p_targets(T, W, H)
    lab = blank(bank, W, H)
    claims = []
    for t, ps in targets.items():
        tpl = template_of(bank, "p", t)
        for p in ps:
            xy = plant_pyramid(lab, bank, W, H, tpl, (p % Wc, p // Wc), linear=True)
            claims.append(dict(kind="best_placement", frame=8 if second else 0, template=t, placement=p, positions=npos[t], xy=xy))
    at = 8 if second else 0
    assert at < n_frames
    zero = blank(bank, W, H)
    frames = [lab if f == at else zero for f in range(n_frames)]
    return Case("p_%dx%d_n%d_%s" % (W, H, n_frames, "second" if second else "first"), bank, W, H, frames, 90.0, claims=claims, instance_frame=at)


P_SETS = {"640x480": ((5, 8), 640, 480), "704x480": ((4, 8), 704, 480)}


def p_cases():
    out = []
    for T, W, H in P_SETS.values():
        for n in P_FRAME_COUNTS:
            out.append(positions(T, W, H, n, False))
            if n > 8:
                out.append(positions(T, W, H, n, True))
    return out


# ---- F: refinement ---------------------------------------------------------------------------------------------------------------------
F_W, F_H, F_T = 320, 240, (5, 8)
F_COUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63)
COARSE_CELL_XY = ((1, 2), (4, 1), (6, 5), (2, 6), (5, 3), (0, 0))


def f_template(nf0_per_mod, seed, T=F_T, w0=None):
    """Level 0: nf features per modality on an 8-column grid of cells, one phase; coarser level(s): six features in one cell (six, so that
    the coarse test still passes a full instance at thresholds up to 95)."""
    rng = np.random.default_rng(seed)
    L = len(T)
    tpl = []
    for l in range(L):
        lv = []
        for m, nf in enumerate(nf0_per_mod):
            if l == 0:
                f = grid_features(nf, T[0], (int(rng.integers(0, T[0])), int(rng.integers(0, T[0]))), rng.integers(0, 8, 8).tolist())
                lv.append((w0 or 8 * T[0], 8 * T[0], f))
            else:
                lv.append((max(1, (w0 or 8 * T[0]) >> l), max(1, (8 * T[0]) >> l), [(x, y, (m + l + 3 * i) % 8) for i, (x, y) in enumerate(COARSE_CELL_XY)]))
        tpl.append(lv)
    return tpl


def f_wave_split():
    """Level-0 feature counts around the wave split 16 * wave < nf, M = 1, 2 and one bank with M = 3: one frame per template, a full instance
    whose last level-0 feature (the one the last live wave holds) answers 3: a wave that is skipped, or run on the wrong rows, changes the sum."""
    cases = []
    for M, counts in ((1, F_COUNTS), (2, F_COUNTS), (3, (17, 33, 63))):
        mods = (CG, DN, CG)[:M]
        bank = make_bank(F_T, mods, {"f": [f_template((nf,) * M if M != 2 else (nf, F_COUNTS[(i + 3) % len(F_COUNTS)]), 300 * M + nf) for i, nf in enumerate(counts)]})
        frames, claims = [], []
        for k in range(len(counts)):
            tpl = template_of(bank, "f", k)
            lab = blank(bank, F_W, F_H)
            resp = {(0, m): [4] * (len(tpl[0][m][2]) - 1) + [3] for m in range(M)}
            xy = plant_pyramid(lab, bank, F_W, F_H, tpl, (5 + k % 3, 4 + k % 2), patch_cell=(8 - k % 2, 8), responses=resp)
            nf = sum(len(tpl[0][m][2]) for m in range(M))
            claims.append(dict(kind="match", frame=k, template=k, xy=xy, best=4 * nf - M, nf=nf))
            frames.append(lab)
        cases.append(Case("f_wave_split_M%d" % M, bank, F_W, F_H, frames, 70.0, claims=claims))
    return cases


F_TIES = {   # patch cells (column, row) of identical instances; the first in row-major order wins
    "two_rows": [(9, 11), (3, 2)],
    "two_lanes_one_row": [(9, 5), (2, 5)],
    "one_lane": [(6, 7), (4, 7)],
    "four": [(12, 12), (1, 12), (12, 1), (1, 1)],
    "corner_0_0": [(0, 0)], "corner_0_15": [(15, 0)], "corner_15_0": [(0, 15)], "corner_15_15": [(15, 15)],
    "corners_tie": [(15, 15), (0, 15), (15, 0), (0, 0)],
}


def f_argmax():
    """One template (three level-0 features in one cell, two modalities), one coarse candidate per frame at cell (9, 7); the level-0 instances
    sit at the patch cells of F_TIES.  Plus a frame whose level 0 is empty (best == 0)."""
    tpl = [[(F_T[0], F_T[0], [(1, 1, 2), (3, 0, 5)]), (F_T[0], F_T[0], [(0, 3, 7)])], [(F_T[1], F_T[1], [(1, 2, 1)]), (F_T[1], F_T[1], [(4, 1, 6)])]]
    bank = make_bank(F_T, (CG, DN), {"f": [tpl]})
    tpl = template_of(bank, "f", 0)
    frames, claims = [], []
    cell = (9, 7)
    x1, y1 = cell[0] * F_T[1] + offset_of(F_T[1]), cell[1] * F_T[1] + offset_of(F_T[1])
    ocx, ocy = patch_origin(bank, F_W, F_H, tpl, 0, x1, y1)
    for name, cells in F_TIES.items():
        lab = blank(bank, F_W, F_H)
        for m in range(2):
            plant(lab[1][m], F_T[1], cell, tpl[1][m][2])
            for pc in cells:
                plant(lab[0][m], F_T[0], (ocx + pc[0], ocy + pc[1]), tpl[0][m][2])
        first = min(cells, key=lambda c: (c[1], c[0]))
        claims.append(dict(kind="tie", frame=len(frames), template=0, coarse_cell=cell, cells=cells, first=first, best=12,
                           xy=((ocx + first[0]) * F_T[0] + offset_of(F_T[0]), (ocy + first[1]) * F_T[0] + offset_of(F_T[0]))))
        frames.append(lab)
    lab = blank(bank, F_W, F_H)
    for m in range(2):
        plant(lab[1][m], F_T[1], cell, tpl[1][m][2])
    claims.append(dict(kind="best_zero", frame=len(frames), template=0, coarse_cell=cell,
                       xy=((ocx - 1) * F_T[0] + offset_of(F_T[0]), (ocy - 1) * F_T[0] + offset_of(F_T[0]))))
    frames.append(lab)
    return [Case("f_argmax_thr60", bank, F_W, F_H, frames, 60.0, claims=claims),
            Case("f_argmax_thr0", bank, F_W, F_H, frames, 0.0, claims=claims)]     # threshold 0: the record upstream emits for best == 0


def around(v):
    v = F32(v)
    return [float(np.nextafter(v, F32(-np.inf))), float(v), float(np.nextafter(v, F32(np.inf)))]


def f_equality():
    """Thresholds at the reference's float32 similarity of a planted best, and one float32 step below and above it.  nf = 4, 16 (the division
    is exact) and 3, 7, 63 (rounded); M = 1: the final test alone.  M = 2: the same three thresholds around the between-modalities bound
    max_partial + 4 * remaining as well, with a best that then passes or fails the final test on its own."""
    cases = []
    for nf in (4, 16, 3, 7, 63):
        bank = make_bank(F_T, (CG,), {"f": [f_template((nf,), 500 + nf)]})
        tpl = template_of(bank, "f", 0)
        best = 4 * nf - max(1, nf // 3)
        resp = lowered([nf], best, [(0, i) for i in range(nf)])
        lab = blank(bank, F_W, F_H)
        xy = plant_pyramid(lab, bank, F_W, F_H, tpl, (6, 5), responses={(0, 0): resp[0]})
        sim = F32(F32(best) * F32(100.0) / F32(4 * nf))
        for i, thr in enumerate(around(sim)):
            cases.append(Case("f_equality_nf%d_%s" % (nf, ("below", "at", "above")[i]), bank, F_W, F_H, [lab], thr,
                              claims=[dict(kind="refine_edge", frame=0, template=0, xy=xy, best=best, nf=nf, sim=float(sim), kept=i < 2)]))
    for nfa, nfb in ((4, 4), (3, 4), (17, 46)):
        bank = make_bank(F_T, (CG, DN), {"f": [f_template((nfa, nfb), 600 + nfa)]})
        tpl = template_of(bank, "f", 0)
        nf = nfa + nfb
        part = 4 * nfa - max(2, nfa)                    # best partial sum behind modality 0
        bound = part + 4 * nfb
        for final in ("full", "short"):                 # modality 1 answers in full (best == bound), or one short of it
            lab = blank(bank, F_W, F_H)
            ra = lowered([nfa], part, [(0, i) for i in range(nfa)])[0]
            rb = [4] * nfb if final == "full" else [3] + [4] * (nfb - 1)
            xy = plant_pyramid(lab, bank, F_W, F_H, tpl, (6, 5), responses={(0, 0): ra, (0, 1): rb})
            best = part + sum(rb)
            bsim = F32(F32(bound) * F32(100.0) / F32(4 * nf))
            for i, thr in enumerate(around(bsim)):
                sim = F32(F32(best) * F32(100.0) / F32(4 * nf))
                cases.append(Case("f_bound_nf%d+%d_%s_%s" % (nfa, nfb, final, ("below", "at", "above")[i]), bank, F_W, F_H, [lab], thr,
                                  claims=[dict(kind="refine_edge", frame=0, template=0, xy=xy, best=best, nf=nf, sim=float(sim), kept=bool(not sim < F32(thr)),
                                               bound=bound)]))
    return cases


def f_clamps():
    """Candidates whose doubled position is clamped at the border and at max_x / max_y; a template wider than the image allows (max_x <
    border: the patch origin goes negative and C++ truncation applies); level-0 features that leave the image after the shift on all four
    sides.  Level 1 is 0xff everywhere, so every placement of every template is a candidate; level 0 is a dense random one-hot image."""
    T = F_T
    # with the origin at -12 cells (-60 px) these leave the image on the left, at the top, on the right and at the bottom, or stay inside
    spread_f = [(30, 100, 1), (200, 30, 2), (10, 10, 3), (390, 100, 5), (100, 300, 6), (0, 0, 7), (150, 120, 0), (379, 299, 4), (380, 150, 2)]
    tpls = [
        [[(40, 40, grid_features(12, T[0], (1, 2), [0, 3, 5]))], [(20, 20, [(0, 0, 1)])]],
        [[(250, 40, grid_features(9, T[0], (0, 0), [1, 6]))], [(125, 20, [(0, 0, 2)])]],          # max_x = 320 - 250 - 40 = 30 < border
        [[(40, 180, spread_f)], [(20, 90, [(0, 0, 3)])]],                                      # max_y = 240 - 180 - 40 = 20 < border
        [[(300, 220, spread_f)], [(8, 8, [(0, 0, 4)])]],                                        # both negative: max_x = -20, max_y = -20
    ]
    bank = make_bank(T, (CG,), {"f": tpls})
    rng = np.random.default_rng(11)
    frames = []
    for f in range(2):
        lab = blank(bank, F_W, F_H)
        full_tile(lab[1][0], T[1])
        lab[0][0][:] = np.where(rng.uniform(0, 1, (F_H, F_W)) < 0.5, 1 << rng.integers(0, 8, (F_H, F_W)), 0).astype(np.uint8)
        frames.append(lab)
    return [Case("f_clamps", bank, F_W, F_H, frames, 30.0, claims=[dict(kind="clamps")])]


def f_depth():
    """L = 1: no refinement loop, the coarse similarity with its + 0.5.  L = 3: two refinement steps (the double-buffered partial sums)."""
    cases = []
    T1 = (8,)
    bank = make_bank(T1, (CG, DN), {"f": [[[(64, 64, grid_features(nf - nf // 2, 8, (2, 3), [1, 4, 6])), (64, 64, grid_features(nf // 2, 8, (5, 1), [0, 7]))]] for nf in (5, 31)]})
    frames, claims = [], []
    for k, nf in enumerate((5, 31)):
        tpl = template_of(bank, "f", k)
        lab = blank(bank, 160, 120)
        per = [len(tpl[0][m][2]) for m in range(2)]
        rt = R.raw_threshold(nf, 80.0)
        for cell, total in zip(((1, 1), (11, 5)), (rt, rt + 1)):
            resp = lowered(per, total, [(m, i) for m in range(2) for i in range(per[m])])
            plant_pyramid(lab, bank, 160, 120, tpl, cell, responses={(0, m): resp[m] for m in range(2)})
            claims.append(dict(kind="coarse_sum", frame=k, template=k, cell=cell, total=total, raw_threshold=rt, candidate=total > rt, tight=False, level=0))
        frames.append(lab)
    cases.append(Case("f_depth_L1", bank, 160, 120, frames, 80.0, claims=claims))
    T3 = (4, 8, 10)
    W = H = 320
    bank = make_bank(T3, (CG, DN), {"f": [f_template((nf, 70 - nf), 700 + nf, T=T3) for nf in (17, 33, 49)]})
    frames, claims = [], []
    for k in range(3):
        tpl = template_of(bank, "f", k)
        lab = blank(bank, W, H)
        resp = {(0, 0): [4] * (len(tpl[0][0][2]) - 1) + [2], (1, 1): [3, 4, 4, 4, 4, 4]}
        xy = plant_pyramid(lab, bank, W, H, tpl, (3 + k, 4), patch_cell=(7 + k, 9 - k), responses=resp)
        claims.append(dict(kind="match", frame=k, template=k, xy=xy, best=4 * 70 - 2, nf=70))
        frames.append(lab)
    cases.append(Case("f_depth_L3", bank, W, H, frames, 70.0, claims=claims))
    return cases


def table_order(bank, W, H):
    """{template: [(modality, feature index)]} in the order of the scoring kernel's block table, decoded from the table itself
    (lmx_debug_bank_tables through test_score_schedule_host.rows_of): an entry is modality * uni_block + label * nib_ori_stride + 4 * (e0 //
    8) with the nibble e0 % 8 in the block's meta word, which identifies the feature."""
    import test_score_schedule_host as host
    t = host.rows_of(bank, W, H)
    g = t["geom"]
    L, M = len(bank.T), len(bank.modalities)
    zero_byte = int(g["nib_zero_off"]) // 4 * 4
    out = {}
    for k in range(len(t["blk"])):
        tpl = template_of(bank, bank.classes[0][0], k)
        key = {}
        for m in range(M):
            for i, (x, y, lab) in enumerate(np.asarray(tpl[L - 1][m][2]).reshape(-1, 3).tolist()):
                key[m, lab, int(R.linear_index(g, x, y))] = (m, i)
        order = []
        for b in range(int(t["sinfo"][k, 3] >> 16 & 0xff)):
            meta = int(t["blk"][k, b, 15])
            for q in range(R.SB_GROUPS):
                for off in t["blk"][k, b, 3 * q:3 * q + 3]:
                    m, r = divmod(int(off), t["uni_block"])
                    if r == zero_byte:
                        continue
                    lab, e = divmod(r, int(g["nib_ori_stride"]))
                    order.append(key[m, lab, e // 4 * 8 + (meta >> 5 * q & 31) // 4])
        assert sorted(order) == sorted(key.values()), k
        out[k] = order
    return out


def s_tight():
    """The pruning bound's equality edge: totals of raw_threshold + 1 with the missing response in the features the table serves first."""
    out = []
    for M in (1, 2):
        order = table_order(s_bank(M), S_W, S_H)
        out += s_thresholds(M, name="s_tight", table_order=order, thresholds=(75.0, 92.0))
    return out


FAMILIES = {
    "r_coarse": lambda: [r_coarse(g) for g in R_COARSE_GEOMS],
    "r_fine": lambda: [r_fine("plain"), r_fine("neighbours")],
    "r_fine_levels3": r_fine_levels3,
    "s_thresholds": lambda: s_thresholds(1) + s_thresholds(2) + s_thresholds(2, S_COUNTS_WIDE, name="s_wide"),
    "s_tight": s_tight,
    "saturated": lambda: [saturated(M) for M in (1, 2, 3)],
    "per_class": lambda: [per_class_edges()],
    "p": p_cases,
    "f_wave_split": f_wave_split,
    "f_argmax": f_argmax,
    "f_equality": f_equality,
    "f_clamps": f_clamps,
    "f_depth": f_depth,
}
_built = {}


def family(name):
    """The cases of a family, built once per process and never modified."""
    if name not in _built:
        _built[name] = FAMILIES[name]()
    return _built[name]
