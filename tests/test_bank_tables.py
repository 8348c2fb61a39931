"""The tables a context uploads for the scoring and refinement kernels (csrc/lmx_bank_tables.hpp), checked on the CPU through
lmx_debug_bank_tables, two ways:
  meaning   every table decoded and compared with the numpy restatement of its documented format (np_restatement.py, from the bank's flat
            arrays alone);
  bytes     FNV-1a digests of every table against tests/golden/bank_tables_digests.json, which the table builder's code BEFORE it became a
            function of its own produced for the same inputs (never regenerate them from the code under test).
Inputs: the banks of four golden cases and one hand-built bank (hand_bank), each at a size whose level 0 gets the banded spread image
and at one where it stays flat, with LMX_LS_FLAT's switch on and off, as the whole bank and as shard 1 of 3."""
import json
import os

import numpy as np
import pytest

import golden_util as G
import np_restatement as R
from linemod_pose_estimation_amd import _lib, meshsynth
from linemod_pose_estimation_amd.bank import DEFAULT_COLOR_GRADIENT, DEFAULT_DEPTH_NORMAL, TemplateBank
from linemod_pose_estimation_amd.detector import NativeBank

MAX_BATCH = 3
TABLES = ("info", "linfo", "coarse_off", "coarse_uni", "coarse_blk", "sinfo", "feat", "feat_count", "summary")   # _lib.LMX_TAB_* order
FEAT_DTYPE = np.dtype([("off", "<u4"), ("x", "<i2"), ("y", "<i2")])
DIGESTS = os.path.join(G.HERE, "golden", "bank_tables_digests.json")


def hand_bank():
    """Three modalities, two levels (T = 4, 8), two classes whose key order is not their insertion order.  Class "m_hand" template 3 has 70
    coarsest-level features (uni_ok = 0), template 4 has 57 spread over all eight nibble classes with leftovers, template 5 has an empty
    modality (and template 3's third one is empty too); coarsest-level features reach x = 32 and 64, y = 48: the image's width and height at
    the two sizes BANKS gives this bank."""
    rng = np.random.default_rng(20260701)
    mods = [dict(DEFAULT_COLOR_GRADIENT), dict(DEFAULT_DEPTH_NORMAL), dict(DEFAULT_COLOR_GRADIENT)]
    bank = TemplateBank(T=[4, 8], modalities=mods)
    special = {3: (40, 30, 0), 4: (25, 20, 12), 5: (7, 0, 0)}
    for cid, n in (("m_hand", 9), ("a_other", 4)):
        rows, feats = [], []
        for t in range(n):
            for l, (xmax, ymax) in enumerate(((128, 96), (65, 49))):
                w, h = int(rng.integers(8, 40)), int(rng.integers(8, 40))
                for m in range(3):
                    fc = special[t][m] if cid == "m_hand" and l == 1 and t in special else int(rng.integers(0, 12))
                    f = np.stack([rng.integers(0, xmax, fc), rng.integers(0, ymax, fc), rng.integers(0, 8, fc)], 1)
                    if l == 1 and fc >= 7:
                        f[:3, 0], f[3:5, 1] = (32, 64, 64), 48
                    rows.append((w, h, l, sum(len(a) for a in feats), fc))
                    feats.append(f)
        bank.classes.append((cid, np.asarray(rows, np.int32), np.concatenate(feats).astype(np.int32)))
    return bank


def _golden(name):
    return G.load(os.path.join(G.HERE, "golden", name + ".npz"))[1]


# name -> (bank, size with a banded level 0 (Wc % 16 == 0, Wc >= 32, Wc != Hc), size without)
BANKS = {
    "case_rgbd_240x160": (lambda: _golden("case_rgbd_240x160"), (320, 240), (80, 160)),
    "case_cg_only_160": (lambda: _golden("case_cg_only_160"), (320, 240), (80, 160)),
    "case_rgbd_two_classes_T48": (lambda: _golden("case_rgbd_two_classes_T48"), (192, 128), (96, 128)),
    "mesh_bank_memoryChip2": (lambda: meshsynth.load_bank("memoryChip2")[0], (640, 480), (80, 480)),
    "hand": (hand_bank, (128, 96), (64, 96)),
}
CONFIGS = [(name, banded, flat, shard) for name in BANKS for banded in (True, False) for flat in (False, True) for shard in ((0, 1), (1, 3))]
_cache = {}


def config_key(name, banded, flat, shard):
    return "%s/%s/%s/shard%dof%d" % (name, "banded_size" if banded else "flat_size", "ls_flat" if flat else "default", shard[0], shard[1])


def tables_of(name, banded, flat, shard):
    """-> (TemplateBank, {table: uint8 bytes}, {table: the library's FNV-1a})."""
    if name not in _cache:
        bank = BANKS[name][0]()
        _cache[name] = (bank, NativeBank.from_bank(bank))
    bank, native = _cache[name]
    w, h = BANKS[name][1 if banded else 2]
    got = [native.debug_tables(k, w, h, MAX_BATCH, shard[0], shard[1], flat) for k in range(len(TABLES))]
    return bank, {t: g[0] for t, g in zip(TABLES, got)}, {t: g[1] for t, g in zip(TABLES, got)}


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def sorted_rows(a, width):
    """Rows as multisets: padded with R.NONE to `width` columns and sorted."""
    a = np.concatenate([a, np.full((a.shape[0], width - a.shape[1]), R.NONE)], 1)
    return np.sort(a, 1)


@pytest.mark.parametrize("name,banded,flat,shard", CONFIGS, ids=[config_key(*c) for c in CONFIGS])
def test_tables_mean_what_their_formats_say(name, banded, flat, shard):
    bank, raw, _ = tables_of(name, banded, flat, shard)
    L, M = len(bank.T), len(bank.modalities)
    W, H = BANKS[name][1 if banded else 2]
    s = raw["summary"].view("<u4").astype(np.int64)
    geom = [dict(zip(R.GEOM_FIELDS, s[8 + 16 * l:24 + 16 * l])) for l in range(L)]
    for l, g in enumerate(geom):
        assert (g["W"], g["H"], g["T"]) == (W >> l, H >> l, bank.T[l]) and (g["Wc"], g["Hc"], g["cells"]) == (g["W"] // g["T"], g["H"] // g["T"], g["W"] // g["T"] * (g["H"] // g["T"]))
    # what the case exists for: level 0 is banded at the banded size unless LMX_LS_FLAT's switch is on, and rows and columns differ there
    assert (geom[0]["ls_bands"] > 0) == (banded and not flat) and geom[L - 1]["ls_bands"] == 0
    if geom[0]["ls_bands"]:
        assert geom[0]["ls_bands"] == geom[0]["Wc"] // 16 and geom[0]["Wc"] != geom[0]["Hc"]
    gc = geom[L - 1]
    F = R.shard_features(bank, *shard)
    n_g = len(F["template_id"])
    assert n_g == sum(e - b for b, e in bank.shard(*shard).values()) and (n_g > 0)
    nf_total = F["count"].sum(2)                                  # [L, G]
    uni_block = MAX_BATCH * gc["nib_mod_stride"]
    assert list(s[:8]) == [n_g, F["count"][L - 1].max(), int(nf_total[L - 1].max() <= 63 and M * uni_block + gc["nib_mod_stride"] < 1 << 27), uni_block, L, M,
                           len(bank.classes), 0]

    # info, linfo, sinfo, feat_count: the shard's templates in class key order, TemplateBank.shard's ranges
    info = raw["info"].view("<i4").reshape(n_g, 4)
    assert np.array_equal(info, np.stack([F["class_index"], F["template_id"], np.zeros(n_g), np.zeros(n_g)], 1))
    pos = np.stack([R.template_positions(geom[l], F["wh"][:, l, 0], F["wh"][:, l, 1]) for l in range(L)], 1)
    linfo = raw["linfo"].view("<i4").reshape(n_g, L, 4)
    assert np.array_equal(linfo, np.stack([F["wh"][:, :, 0], F["wh"][:, :, 1], nf_total.T, pos], 2))
    assert np.array_equal(raw["feat_count"].reshape(L, n_g, M), F["count"])
    sinfo = raw["sinfo"].view("<u4").reshape(n_g, 4).astype(np.int64)
    assert np.array_equal(sinfo[:, :3], np.stack([pos[:, L - 1], nf_total[L - 1], F["class_index"]], 1))

    # feat: flat or banded entries, padding at the level's zero run, the count in entry 63
    feat = raw["feat"].view(FEAT_DTYPE).reshape(L, n_g, M, R.FEAT_STRIDE)
    for l, g in enumerate(geom):
        off, ex, ey = R.feat_entries(g, F["x"][l], F["y"][l], F["label"][l], F["valid"][l], F["count"][l])
        assert np.array_equal(feat[l]["off"], off) and np.array_equal(feat[l]["x"], ex) and np.array_equal(feat[l]["y"], ey), l

    # coarse_off: (dword index << 3) | (e0 & 7); features outside the image and padding = the zero run
    x, y, label, valid = (F[k][L - 1] for k in ("x", "y", "label", "valid"))
    byte, nib = R.coarse_address(gc, x, y, label, valid)
    coarse_off = raw["coarse_off"].view("<u4").reshape(n_g, M, R.FEAT_STRIDE).astype(np.int64)
    assert np.array_equal(coarse_off, byte // 4 << 3 | nib)
    zero_byte = gc["nib_zero_off"] // 4 * 4
    outside = valid & ((x >= gc["W"]) | (y >= gc["H"]))
    assert np.all(coarse_off[outside] == zero_byte // 4 << 3) and np.all(coarse_off[~valid] == zero_byte // 4 << 3)
    if name == "hand":
        assert (valid & (x == gc["W"])).any() and (valid & (y == gc["H"])).any() and not (F["count"][L - 1] > 0).all()

    # coarse_uni / coarse_blk of the templates with at most 63 coarsest-level features; the others keep default rows
    ok = nf_total[L - 1] <= 63
    uni = raw["coarse_uni"].view("<u4").reshape(n_g, R.FEAT_STRIDE).astype(np.int64)
    blk = raw["coarse_blk"].view("<u4").reshape(n_g, R.SB_MAX_BLOCKS, R.SB_BLOCK).astype(np.int64)
    assert np.all(uni[~ok] == zero_byte // 4 << 3) and np.all(blk[~ok] == 0) and np.all(sinfo[~ok, 3] == 0)
    if name == "hand" and shard == (0, 1):
        assert (~ok).sum() == 1
    # the template's features in the final form (byte offset from modality 0's block | 4 * nibble << 27), modality m's block m * uni_block on
    real = np.where(valid, byte + np.arange(M)[None, :, None] * uni_block | 4 * nib << 27, R.NONE).reshape(n_g, -1)[ok]
    nibs, val, nf = nib.reshape(n_g, -1)[ok], valid.reshape(n_g, -1)[ok], nf_total[L - 1][ok]
    n_fast, group_class, group_real, n_grps = R.coarse_group_plan(nibs, val)
    uni, blk, groups = uni[ok], blk[ok], sinfo[ok, 3]
    n_ok, cols = len(uni), np.arange(R.FEAT_STRIDE - 1)
    # unified row: entries [0, nf) are the features, the rest of 0..62 points at the zero run with shift 0
    is_real = cols[None, :] < nf[:, None]
    assert np.array_equal(sorted_rows(np.where(is_real, uni[:, :63], R.NONE), real.shape[1] + 63), sorted_rows(real, real.shape[1] + 63))
    assert np.all(uni[:, :63][~is_real] == zero_byte)
    assert np.array_equal(uni[:, 63], n_fast | (nf + 2) // 3 << 8) and np.array_equal(groups & 0xffff, uni[:, 63])
    # ... its fast groups hold one shift each: the nibble classes round robin, from class 0
    shifts = (uni[:, :63] >> 27).reshape(n_ok, 21, 3)
    fast = np.arange(21)[None, :] < n_fast[:, None]
    assert np.all(shifts[fast] == 4 * group_class[:, :21][fast][:, None])
    # block row: blocks of 5 groups x 3 byte offsets, then the groups' shifts (5 bits each) | real features consumed so far << 25
    n_blocks = groups >> 16
    assert np.array_equal(n_blocks, (n_grps + R.SB_GROUPS - 1) // R.SB_GROUPS) and n_grps.max(initial=0) <= R.SB_GROUPS * R.SB_MAX_BLOCKS
    offs, meta = blk[:, :, :15].reshape(n_ok, 30, 3), blk[:, :, 15]
    gi = np.arange(30)
    used = gi[None, :] < n_grps[:, None]
    grp_shift = meta[:, gi // R.SB_GROUPS] >> 5 * (gi % R.SB_GROUPS) & 31
    assert np.all(grp_shift[used] == 4 * group_class[:, :30][used])                 # one shift per group: fast ones first, then a group per leftover class
    pads = np.where((np.arange(3)[None, None, :] >= group_real[:, :30, None]) & used[:, :, None], zero_byte | grp_shift[:, :, None] << 27, R.NONE).reshape(n_ok, -1)
    assert np.array_equal(sorted_rows(np.where(used[:, :, None], offs | grp_shift[:, :, None] << 27, R.NONE).reshape(n_ok, -1), real.shape[1] + 180),
                          sorted_rows(np.concatenate([real, pads], 1), real.shape[1] + 180))
    assert np.all(offs[~used] == zero_byte)                                           # unused group slots and ...
    block_used = np.arange(R.SB_MAX_BLOCKS)[None, :] < n_blocks[:, None]
    assert np.all(meta[~block_used] == zero_byte)                                     # ... unused blocks point at the zero run
    consumed = np.where(block_used, meta >> 25, nf[:, None])
    want = np.concatenate([np.zeros((n_ok, 1), np.int64), np.cumsum(group_real[:, :30], 1)], 1)[:, [min(30, 5 * (b + 1)) for b in range(R.SB_MAX_BLOCKS)]]
    assert np.all(np.diff(consumed, axis=1) >= 0) and np.all(consumed[:, -1] == nf) and np.array_equal(consumed, np.where(block_used, want, nf[:, None]))
    assert np.all(consumed[np.arange(n_ok), np.maximum(n_blocks, 1) - 1][n_blocks > 0] == nf[n_blocks > 0])
    # what the cases exist for: padded groups, several blocks, every nibble class with leftovers in several of them
    if n_ok:
        assert ((group_real > 0) & (group_real < 3)).any() and n_blocks.max() > 1 and (n_fast > 8).any()
    if name == "hand" and banded:   # at the other size most of the bank's coarsest-level features lie outside the image
        cnt = np.stack([(val & (nibs == k)).sum(1) for k in range(8)], 1)
        assert ((cnt > 0).all(1) & ((cnt % 3 > 0).sum(1) >= 3)).any()


@pytest.mark.parametrize("name,banded,flat,shard", CONFIGS, ids=[config_key(*c) for c in CONFIGS])
def test_tables_equal_the_recorded_digests(name, banded, flat, shard):
    with open(DIGESTS) as f:
        want = json.load(f)[config_key(name, banded, flat, shard)]
    _, raw, digest = tables_of(name, banded, flat, shard)
    assert {t: "%016x" % digest[t] for t in TABLES} == want
    assert fnv1a(raw["sinfo"]) == digest["sinfo"] and fnv1a(raw["summary"]) == digest["summary"]   # the library's hash is FNV-1a 64 of the bytes it returns


def test_hook_refuses_bad_arguments():
    native = NativeBank.from_bank(hand_bank())
    n = _lib.C.c_size_t()
    call = lambda *a: _lib.lib().lmx_debug_bank_tables(native.h, *a, None, 0, _lib.C.byref(n), None)
    assert call(128, 96, 1, 0, 1, 0, _lib.LMX_TAB_INFO) == _lib.LMX_OK and n.value == 13 * 16
    assert call(128, 96, 1, 0, 1, 0, 99) == _lib.LMX_ERR_INVALID_ARG
    assert call(128, 96, 1, 3, 3, 0, _lib.LMX_TAB_INFO) == _lib.LMX_ERR_INVALID_ARG
    assert call(130, 96, 1, 0, 1, 0, _lib.LMX_TAB_INFO) == _lib.LMX_ERR_SHAPE   # not a multiple of T: lmx_ctx_create's error
    out = np.zeros(8, np.uint8)
    assert _lib.lib().lmx_debug_bank_tables(native.h, 128, 96, 1, 0, 1, 0, _lib.LMX_TAB_INFO, out.ctypes.data, out.nbytes, None, None) == _lib.LMX_ERR_INVALID_ARG
