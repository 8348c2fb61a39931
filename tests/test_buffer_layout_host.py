"""The byte layout of the spread and response buffers (LevelGeom in csrc/lmx_bank_tables.hpp), pads included, on the CPU:
  round trip    the expected blocks of np_restatement.py (spread_block, nibble_block, byte_block), un-banded and unpacked the way the debug
                read does it, give back the oracle's arrays;
  sensitivity   first_difference names the kind of place of one flipped byte in a COPY of an expected allocation (data only);
  reach         what k_refine can address, from the feature table and the geometry alone: every patch lies inside its block, the patches of
                padded and out-of-image entries lie in bytes the layout keeps zero, and a valid entry's patch holds what upstream's
                similarityLocal reads (flat element lm_index + r * Wc + c, zero past the end).
The geometry comes from LMX_TAB_SUMMARY as in test_bank_tables.py.  tests/test_gpu_buffer_bytes.py compares the device's allocations with the
same expected blocks.  No byte of a band's row 0 is left out: the layout's formula gives every one of them (zero, except the last band's
right half, which holds the first 16 elements)."""
import numpy as np
import pytest

import np_restatement as R
import test_bank_tables as TB
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd.bank import DEFAULT_COLOR_GRADIENT, TemplateBank
from linemod_pose_estimation_amd.detector import NativeBank
from oracle import oracle as o


def geometry_of(native, W, H, max_batch=1, ls_flat=False):
    """-> ([LevelGeom as a dict of R.GEOM_FIELDS per level], the summary's first eight words)."""
    s = native.debug_tables(_lib.LMX_TAB_SUMMARY, W, H, max_batch, 0, 1, ls_flat)[0].view("<u4").astype(np.int64)
    L = int(s[4])
    return [dict(zip(R.GEOM_FIELDS, (int(v) for v in s[8 + 16 * l:24 + 16 * l]))) for l in range(L)], s[:8]


def tiny_bank(T, n_mod=1):
    """One pyramid with one feature per template: the geometry does not depend on more."""
    L = len(T)
    bank = TemplateBank(T=list(T), modalities=[dict(DEFAULT_COLOR_GRADIENT) for _ in range(n_mod)])
    rows = np.asarray([(8, 8, l, l * n_mod + m, 1) for l in range(L) for m in range(n_mod)], np.int32)
    bank.classes.append(("obj", rows, np.tile(np.asarray([[1, 1, 0]], np.int32), (L * n_mod, 1))))
    return bank


# (T, W, H, LMX_LS_FLAT, bands of level 0): banded and flat level 0, T in {4, 5, 8, 10} at the finer and at the coarsest level, odd Wc at both
LAYOUT_CASES = [((4, 8), 128, 96, False, 2), ((5, 8), 240, 160, False, 3), ((8, 4), 256, 128, False, 2), ((10, 5), 320, 160, False, 2),
                ((5, 8), 240, 160, True, 0), ((5, 10), 80, 160, False, 0), ((5, 8), 80, 160, False, 0), ((8, 10), 120, 80, False, 0),
                ((4, 5), 140, 80, False, 0), ((4, 8, 10), 320, 320, False, 5)]


def random_labels(rng, H, W):
    return np.where(rng.uniform(0, 1, (H, W)) < 0.5, 1 << rng.integers(0, 8, (H, W)), 0).astype(np.uint8)


def oracle_arrays(rng, g):
    """Random labels through the oracle's spread, response maps and linearize -> (flat spread image [T * T, cells], memories [8, T * T, cells])."""
    sp = o.spread(random_labels(rng, g["H"], g["W"]), g["T"])
    rm = o.response_maps(sp)
    return o.linearize(sp, g["T"]), np.stack([o.linearize(rm[k], g["T"]) for k in range(8)])


@pytest.mark.parametrize("T,W,H,ls_flat,bands", LAYOUT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_expected_blocks_read_back_as_the_oracles_arrays(T, W, H, ls_flat, bands):
    geom, _ = geometry_of(NativeBank.from_bank(tiny_bank(T)), W, H, 1, ls_flat)
    rng = np.random.default_rng(W * 1000 + H + T[0])
    assert geom[0]["ls_bands"] == bands
    for l, g in enumerate(geom):
        n = g["T"] ** 2 * g["cells"]
        flat, lm = oracle_arrays(rng, g)
        assert flat.shape == (g["T"] ** 2, g["cells"]) and (flat != 0).mean() > 0.5
        if l < len(geom) - 1:
            block, kind = R.spread_block(g, flat)
            assert len(block) == g["ls_stride"] and np.array_equal(R.unband_spread_block(g, block), flat.reshape(-1))
            count = np.bincount(kind, minlength=len(R.BYTE_KINDS))
            if g["ls_bands"]:   # every cell twice; the wrapped copies are all but the first row's first 16 columns, which band row 0 holds too
                rows = g["T"] ** 2 * g["Hc"]
                assert count[R.K_OWN] == n and count[R.K_DUP] + count[R.K_WRAP] == n and count[R.K_WRAP] == 16 * rows and count[R.K_PAYLOAD] == 0
                assert count[R.K_ZERO_ROW] == g["ls_bands"] * (rows + 17) * 32 - 2 * n
                last = (g["ls_bands"] - 1) * g["ls_band_stride"]
                assert np.array_equal(block[last + 16:last + 32], flat.reshape(-1)[:16]) and not block[:16].any() and not block[last:last + 16].any()
                z = g["ls_zero_off"]   # the zero run of the tables: 16 band rows behind the image, band 0
                assert z == (rows + 1) * 32 and np.all(kind[z:z + 16 * 32] == R.K_ZERO_ROW)
            else:
                assert count[R.K_PAYLOAD] == n and np.array_equal(block[:n], flat.reshape(-1)) and g["ls_zero_off"] == n
            assert not block[kind >= R.K_ZERO_ROW].any()
        else:
            nb, nk = R.nibble_block(g, lm)
            assert len(nb) == g["nib_mod_stride"] and np.array_equal(R.unpack_nibble_block(g, nb), lm.reshape(8, n))
            assert not nb[nk != R.K_PAYLOAD].any() and (nk == R.K_PAYLOAD).sum() == 8 * ((n + 1) // 2)
            bb, bk = R.byte_block(g, lm)
            assert len(bb) == g["mod_stride"] and not bb[bk != R.K_PAYLOAD].any()
            for k in range(8):
                assert np.array_equal(bb[k * g["ori_stride"]:k * g["ori_stride"] + n], lm[k].reshape(-1))
            # the scoring kernels' zero run, and what k_pack_nibbles reads behind an orientation's payload (it packs groups of 8 up to n + 8)
            assert np.all(nk[g["nib_zero_off"]:g["nib_zero_off"] + g["cells"] // 2 + 2048] == R.K_ZERO_RUN) and g["nib_zero_off"] % 4 == 0
            assert g["ori_stride"] - n >= 16 and g["nib_ori_stride"] - (n + 1) // 2 >= 8


def _allocations():
    """Two-frame allocations of a banded spread image, a flat one, nibble memories and byte-wide memories."""
    rng = np.random.default_rng(5)
    out = {}
    for name, (T, W, H) in {"banded": ((5, 8), 240, 160), "flat": ((5, 8), 80, 160)}.items():
        geom, _ = geometry_of(NativeBank.from_bank(tiny_bank(T)), W, H, 2)
        out[name] = R.allocation([R.spread_block(geom[0], oracle_arrays(rng, geom[0])[0]) for _ in range(2)])
        if name == "banded":
            out["nibbles"] = R.allocation([R.nibble_block(geom[1], oracle_arrays(rng, geom[1])[1]) for _ in range(2)])
            out["bytes"] = R.allocation([R.byte_block(geom[1], oracle_arrays(rng, geom[1])[1]) for _ in range(2)])
    return out


@pytest.mark.parametrize("name,kinds", [
    ("banded", ("own half", "duplicate half", "wrapped duplicate", "zero row", "zero run", "tail")),
    ("flat", ("payload", "zero run", "tail")),
    ("nibbles", ("payload", "zero run", "inter-orientation pad", "block tail", "tail")),
    ("bytes", ("payload", "zero run", "inter-orientation pad", "block tail", "tail"))])
def test_the_comparer_names_the_place_of_one_wrong_byte(name, kinds):
    want, kind = _allocations()[name]
    assert R.first_difference(want.copy(), want, kind) is None
    assert sorted(R.BYTE_KINDS[k] for k in np.unique(kind)) == sorted(kinds)
    for k in kinds:
        at = np.flatnonzero(kind == R.BYTE_KINDS.index(k))
        for i in (at[0], at[len(at) // 2], at[-1]):   # also in the second frame's block
            got = want.copy()
            got[i] ^= 0x10
            assert R.first_difference(got, want, kind) == (k, i, want[i] ^ 0x10, want[i]), (k, i)
    # the first of several wrong bytes is the one reported
    got = want.copy()
    got[[len(got) - 1, 40]] ^= 1
    assert R.first_difference(got, want, kind)[1] == 40


# ---- what k_refine can address ------------------------------------------------------------------------------------------------------
def reader_address(g, row, col):
    """Where the patch of an element at (row, column) of the level's matrix starts in a block: the flat index, or, banded, the band of the
    column (LevelGeom: band k keeps columns 16 k .. 16 k + 31 of every row in 32 bytes, matrix row r in band row r + 1)."""
    if not g["ls_bands"]:
        return row * g["Wc"] + col
    return (col >> 4) * g["ls_band_stride"] + (row + 1) * 32 + (col & 15)


def patch_bytes(g, address):
    """Offsets [..., 16, 16] of the 16 rows x 16 bytes read from `address` on."""
    r, c = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    return np.asarray(address)[..., None, None] + r * (32 if g["ls_bands"] else g["Wc"]) + c


def trunc_div(a, b):
    """C++ integer division (toward zero)."""
    return np.sign(a) * (np.abs(a) // b)


def reachable_origins(geom, wh, axis):
    """Per finer level the cell origins (upstream's x / T - 8) the refinement can reach along one axis (0: x, 1: y) for a template of sizes
    wh [L, 2], from every cell of the coarsest level: x = 2 x' + 1, clamped to [8 T, size - template - 8 T] (max first, then min), and the
    next level starts from any of the 16 cells of the patch.  SURVEY.md A.9 / np_restatement.match."""
    L = len(geom)
    gc = geom[L - 1]
    Tc = gc["T"]
    pos = np.arange(gc["Wc" if axis == 0 else "Hc"]) * Tc + Tc // 2 + (Tc % 2 - 1)
    out = [None] * (L - 1)
    for l in range(L - 2, -1, -1):
        g = geom[l]
        T, size = g["T"], g["W" if axis == 0 else "H"]
        x = 2 * pos + 1
        x = np.minimum(np.maximum(x, 8 * T), size - int(wh[l][axis]) - 8 * T)
        out[l] = np.unique(trunc_div(x, T) - 8)
        pos = np.unique((out[l][:, None] + np.arange(16)[None, :]) * T + T // 2 + (T % 2 - 1))
    return out


REACH_CONFIGS = [(name, banded, flat) for name in TB.BANKS for banded, flat in ((True, False), (False, False), (True, True))]


@pytest.mark.parametrize("name,banded,flat", REACH_CONFIGS, ids=["%s/%s%s" % (n, "banded_size" if b else "flat_size", "/ls_flat" if f else "") for n, b, f in REACH_CONFIGS])
def test_refinement_patches_stay_inside_and_read_what_upstream_reads(name, banded, flat):
    bank, raw, _ = TB.tables_of(name, banded, flat, (0, 1))
    L, M = len(bank.T), len(bank.modalities)
    s = raw["summary"].view("<u4").astype(np.int64)
    geom = [dict(zip(R.GEOM_FIELDS, (int(v) for v in s[8 + 16 * l:24 + 16 * l]))) for l in range(L)]
    F = R.shard_features(bank, 0, 1)
    n_g = len(F["template_id"])
    feat = raw["feat"].view(TB.FEAT_DTYPE).reshape(L, n_g, M, R.FEAT_STRIDE)
    n_valid = n_outside = 0
    for l in range(L - 1):
        g = geom[l]
        T, Wc, Hc = g["T"], g["Wc"], g["Hc"]
        n, rows = T * T * g["cells"], T * T * Hc
        assert (g["ls_bands"] > 0) == (banded and not flat and l == 0) or l > 0
        idx, kind = R.spread_block_index(g)
        # 1. the layout: the patch of EVERY element of the matrix lies inside the block and holds upstream's flat elements, zero past the end
        for r0 in range(0, rows, 256):
            row, col = np.meshgrid(np.arange(r0, min(rows, r0 + 256)), np.arange(Wc), indexing="ij")
            at = patch_bytes(g, reader_address(g, row, col))
            assert at.min() >= 0 and at.max() < g["ls_stride"]
            e = (row * Wc + col)[..., None, None] + np.arange(16)[:, None] * Wc + np.arange(16)[None, :]
            assert np.array_equal(idx[at], np.where(e < n, e, -1))
        # 2. padded entries and entries that leave the image read the zero run: all of its patch is bytes the layout keeps zero
        at = patch_bytes(g, g["ls_zero_off"])
        assert at.max() < g["ls_stride"] and np.all(idx[at] == -1) and np.all(kind[at] >= R.K_ZERO_ROW)
        # 3. the table: for every template and every reachable origin, a valid entry moved by the origin is upstream's element
        x, y, label, exists = (F[k][l] for k in ("x", "y", "label", "valid"))       # [G, M, 64]
        off = feat[l]["off"].astype(np.int64)
        assert np.array_equal(off >> 29, np.where(exists, label, 0)) and np.all((off & 0x1fffffff)[~exists] == g["ls_zero_off"])
        for t in range(n_g):
            ocx, ocy = (reachable_origins(geom, F["wh"][t], a)[l] for a in (0, 1))
            fx, fy = x[t][..., None] + ocx * T, y[t][..., None] + ocy * T            # [M, 64, nx], [M, 64, ny]: upstream's shifted feature
            vx, vy = exists[t][..., None] & (fx >= 0) & (fx < g["W"]), exists[t][..., None] & (fy >= 0) & (fy < g["H"])
            grid = (y[t] % T) * T + x[t] % T                                         # a shift by whole cells keeps the grid
            want_col = fx // T
            want_row = grid[..., None] * Hc + fy // T
            low = (off[t] & 0x1fffffff)[..., None]
            if g["ls_bands"]:
                got_col, got_row = (low & 0xfff) + ocx, (low >> 12) + ocy
                assert np.array_equal(got_col[vx], want_col[vx]) and np.array_equal(got_row[vy], want_row[vy])
            else:   # flat element index + ocy * Wc + ocx, both axes at once
                got = low[..., None] + ocx[:, None] + ocy[None, :] * Wc
                want = (grid * g["cells"])[..., None, None] + (fy // T)[:, :, None, :] * Wc + want_col[..., None]   # accessLinearMemory of the shifted feature
                v = vx[..., None] & vy[:, :, None, :]
                assert np.array_equal(got[v], want[v])
            # a valid entry's element lies in the matrix, so that 1. covers its patch
            assert np.all((want_col[vx] >= 0) & (want_col[vx] < Wc)) and np.all((want_row[vy] >= 0) & (want_row[vy] < rows))
            n_valid += int(vx.any(2).sum())
            n_outside += int((exists[t][..., None] & ~vx).sum())
    assert n_valid > 0
    if name == "hand":   # features up to x = 127 in a 64-wide image (the flat size), or shifted out of it by the clamped origins
        assert n_outside > 0
