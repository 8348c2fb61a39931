"""The schedule of k_score_coarse_sb's bound tests, checked on the CPU against the tables the pure builder emits (lmx_debug_bank_tables).

Block 0 of a template's row (15 features) is loaded whole and tested once.  Every later block is processed in SEGMENTS of whole groups
(3 features), each followed by the exact bound test  S >= raw_threshold + 1 - 4 * (nf - consumed).  The table only knows the real
features consumed through the END of a block (meta >> 25), so after q of the block's 5 groups the kernel uses the lower bound
consumed_end - 3 * (5 - q): each later group holds at most 3.

  bound safety   that lower bound never exceeds the true count of real features in the row's first 5 b + q groups, and is >= 0 wherever a
                 test is issued (need > 0), for rows of 62, 30, 17 and 3 coarsest-level features, single-modality banks and a template
                 with an empty modality
  exactness      a numpy restatement of the segmented pass (504-placement chunks of 63 lanes x 8 placements, per-lane alive flags, a chunk
                 stops when no lane is alive) over the oracle's coarsest-level linear memories returns the placements of the plain full sum,
                 for every template and every threshold 50, 53, ..., 98; and the inputs reach both edges of a mid-block test: a placement
                 with S == need (kept) and a chunk whose best live placement has S == need - 1 (the chunk stops)"""
import os
import re

import numpy as np
import pytest

import np_restatement as R
from linemod_pose_estimation_amd import _lib, synth
from linemod_pose_estimation_amd.detector import NativeBank
from oracle import oracle as o

# groups per segment in the blocks behind the first one, read from the kernel's source so that the restatement follows the kernel
with open(os.path.join(_lib.CSRC, "lmx_kernels.hip")) as _f:
    _SEG0 = int(re.search(r"constexpr int SB_SEG0 = (\d+);", _f.read()).group(1))
SEGMENTS = (_SEG0, R.SB_GROUPS - _SEG0)
assert 0 < _SEG0 < R.SB_GROUPS
CHUNK_LANES, LANE_POS = 63, 8   # a chunk: 63 lanes x 8 placements (one dword of nibbles per lane)
THRESHOLDS = tuple(range(50, 99, 3))
W, H = 640, 480


def raw_threshold(nf, thr):
    return int(np.float32(2 * nf) + np.float32(thr) / np.float32(100.0) * np.float32(2 * nf) + np.float32(0.5))


def rows_of(bank, width=W, height=H):
    """The builder's block rows for a one-frame context: -> dict(geom of the coarsest level, uni_block, sinfo [G, 4], blk [G, 6, 16])."""
    native = NativeBank.from_bank(bank)
    tab = lambda k: native.debug_tables(k, width, height, 1, 0, 1, False)[0]
    s = tab(_lib.LMX_TAB_SUMMARY).view("<u4").astype(np.int64)
    L = len(bank.T)
    geom = dict(zip(R.GEOM_FIELDS, s[8 + 16 * (L - 1):24 + 16 * (L - 1)]))
    n_g = int(s[0])
    assert s[2] == 1    # every template has at most 63 coarsest-level features: the bank qualifies for the block table
    return dict(geom=geom, uni_block=int(s[3]), sinfo=tab(_lib.LMX_TAB_SINFO).view("<u4").reshape(n_g, 4).astype(np.int64),
                blk=tab(_lib.LMX_TAB_COARSE_BLK).view("<u4").reshape(n_g, R.SB_MAX_BLOCKS, R.SB_BLOCK).astype(np.int64))


def without_modality(bank, template, modality):
    """`bank` with the coarsest-level features of one template's modality removed."""
    L, M = len(bank.T), len(bank.modalities)
    cid, t, f = bank.classes[0]
    t = t.copy()
    t[(template * L + L - 1) * M + modality, 4] = 0
    bank.classes[0] = (cid, t, f)
    return bank


def mk(nf, mods, seed, n=12):
    return synth.make_bank(n, modalities=mods, T=(5, 8), seed=seed, num_features=nf, size_range=(30.0, 80.0))


BOUND_BANKS = {
    "rgbd_62": (lambda: mk(63, ("ColorGradient", "DepthNormal"), 41), {62}),
    "rgbd_30": (lambda: mk(30, ("ColorGradient", "DepthNormal"), 42), {30}),
    "color_only_17": (lambda: mk(35, ("ColorGradient",), 43), {17}),
    "depth_only_3": (lambda: mk(6, ("DepthNormal",), 44), {3}),
    "rgbd_62_template_2_without_depth": (lambda: without_modality(mk(63, ("ColorGradient", "DepthNormal"), 45), 2, 1), {62, 31}),
}


@pytest.mark.parametrize("name", list(BOUND_BANKS))
def test_mid_block_bound_never_overcounts(name):
    make, totals = BOUND_BANKS[name]
    bank = make()
    t = rows_of(bank)
    L = len(bank.T)
    F = R.shard_features(bank, 0, 1)
    x, y, label, valid = (F[k][L - 1] for k in ("x", "y", "label", "valid"))
    _, nib = R.coarse_address(t["geom"], x, y, label, valid)
    n_g = len(t["blk"])
    _, _, group_real, n_grps = R.coarse_group_plan(nib.reshape(n_g, -1), valid.reshape(n_g, -1))
    true_consumed = np.concatenate([np.zeros((n_g, 1), np.int64), np.cumsum(group_real, 1)], 1)   # [G, groups + 1]: real features in the first k groups
    nf = t["sinfo"][:, 1]
    assert set(nf.tolist()) == totals and np.array_equal(nf, F["count"][L - 1].sum(1))
    n_blocks = t["sinfo"][:, 3] >> 16 & 0xff
    assert np.array_equal(n_blocks, (n_grps + R.SB_GROUPS - 1) // R.SB_GROUPS)
    checked = undercounts = 0
    for g in range(n_g):
        for b in range(int(n_blocks[g])):
            consumed_end = int(t["blk"][g, b, 15] >> 25)
            assert consumed_end == true_consumed[g, 5 * (b + 1)]              # the table's count is the plan's
            if b == 0:
                continue
            for q in range(1, R.SB_GROUPS + 1):
                bound = consumed_end - 3 * (R.SB_GROUPS - q)
                assert bound <= true_consumed[g, 5 * b + q], (g, b, q)
                undercounts += bound < true_consumed[g, 5 * b + q]
                for thr in THRESHOLDS + (100,):
                    need = raw_threshold(int(nf[g]), thr) + 1 - 4 * (int(nf[g]) - bound)
                    if need > 0:                                               # the kernel issues the test
                        assert bound >= 0, (g, b, q, thr)
                checked += 1
    if max(totals) > 15:
        assert checked > 0
    if name == "color_only_17":
        assert undercounts > 0    # a second block that is almost all padding: the bound is loose there, and must be on the safe side


# ---- exactness ------------------------------------------------------------------------------------------------------------------------
def group_rows(t, g, flat, cells):
    """Template g's row as the kernel reads it: -> (sums [groups, positions rounded up to whole lanes] of the three entries of every group,
    decoded from the table's byte offsets and shifts; consumed_end per block)."""
    geom, pos = t["geom"], -(-int(t["sinfo"][g, 0]) // LANE_POS) * LANE_POS
    n_blocks = int(t["sinfo"][g, 3] >> 16 & 0xff)
    zero_byte = geom["nib_zero_off"] // 4 * 4
    out, consumed_end = [], []
    for b in range(n_blocks):
        meta = int(t["blk"][g, b, 15])
        consumed_end.append(meta >> 25)
        for q in range(R.SB_GROUPS):
            s = np.zeros(pos, np.int32)
            for off in t["blk"][g, b, 3 * q:3 * q + 3]:
                m, r = divmod(int(off), t["uni_block"])
                if r == zero_byte:
                    continue
                lab, e = divmod(r, int(geom["nib_ori_stride"]))
                assert lab < 8 and e % 4 == 0
                e0 = e // 4 * 8 + (meta >> 5 * q & 31) // 4
                s += flat[m][lab][e0:e0 + pos]
            out.append(s)
    return np.stack(out), consumed_end


def segmented_pass(rows, pos, consumed_end, nf, raw_thr, stats, need_offset=0):
    """The kernel's pass over one template's `pos` placements -> boolean [pos]: the placements it would append.  need_offset = 1 is the
    bound one too strict (tests/test_label_cases_host.py: the mutant that must lose a candidate)."""
    chunk_pos = CHUNK_LANES * LANE_POS
    passing = np.zeros(pos, bool)
    for c0 in range(0, pos, chunk_pos):
        n = min(chunk_pos, pos - c0)
        n8 = min(chunk_pos, rows.shape[1] - c0)
        S = np.zeros(chunk_pos, np.int32)
        real = np.arange(chunk_pos) < n
        alive = real.reshape(CHUNK_LANES, LANE_POS).any(1)        # a lane starts alive if its first placement exists
        on = True
        for b, end in enumerate(consumed_end):
            for g0, ng in ([(0, R.SB_GROUPS)] if b == 0 else zip(np.cumsum((0,) + SEGMENTS[:-1]), SEGMENTS)):
                S[:n8] += rows[5 * b + g0:5 * b + g0 + ng, c0:c0 + n8].sum(0)
                need = raw_thr + 1 - 4 * (nf - (end - 3 * (R.SB_GROUPS - g0 - ng))) + need_offset
                if need <= 0:
                    continue
                # dead lanes keep accumulating and are never revived; the placements of the last lane behind the template's last one
                # read the cells that follow, as the kernel's lane does -- they are masked at the append only
                lanes = S.reshape(CHUNK_LANES, LANE_POS)
                mid = b > 0 and g0 + ng < R.SB_GROUPS
                if mid:
                    stats["equal"] += int(((lanes == need) & alive[:, None] & real.reshape(CHUNK_LANES, LANE_POS)).sum())
                real_alive = alive[:, None] & real.reshape(CHUNK_LANES, LANE_POS)      # placements that exist, in lanes still alive
                best = lanes[real_alive].max()
                alive = alive & (lanes >= need).any(1)
                if not alive.any():
                    if mid and best == need - 1:   # the chunk's best real placement misses the bound by one
                        stats["last_one_short"] += 1
                    on = False
                    break
            if not on:
                break
        if on:
            passing[c0:c0 + n] = (np.repeat(alive, LANE_POS) & (S > raw_thr))[:n]
    return passing


EXACT_BANKS = {
    "rgbd_62": (lambda: synth.make_bank(40, T=(5, 8), seed=20260901, num_features=63, size_range=(30.0, 80.0)), 7301),
    "color_only_17": (lambda: synth.make_bank(40, modalities=("ColorGradient",), T=(5, 8), seed=20260902, num_features=35, size_range=(30.0, 80.0)), 7302),
}


@pytest.mark.parametrize("name", list(EXACT_BANKS))
def test_segmented_pass_returns_the_full_sums_placements(name):
    make, scene_seed = EXACT_BANKS[name]
    bank = make()
    t = rows_of(bank)
    L, M, T = len(bank.T), len(bank.modalities), bank.T[-1]
    cells = int(t["geom"]["cells"])
    sources, _ = synth.make_scene(bank, W, H, seed=scene_seed)
    od = o.OracleDetector(bank)
    od.match(sources, 90.0)
    flat = [np.concatenate([od.linear_memory(L - 1, m, (H >> (L - 1), W >> (L - 1))).astype(np.int32).reshape(8, -1),
                            np.zeros((8, cells + 8 * CHUNK_LANES * LANE_POS), np.int32)], 1) for m in range(M)]
    stats = {"equal": 0, "last_one_short": 0}
    n_pass = 0
    for g in range(len(t["blk"])):
        rows, consumed_end = group_rows(t, g, flat, cells)
        nf = int(t["sinfo"][g, 1])
        assert consumed_end[-1] == nf
        pos = int(t["sinfo"][g, 0])
        full = rows[:, :pos].sum(0)
        assert full.max() <= 4 * nf
        for thr in THRESHOLDS:
            raw_thr = raw_threshold(nf, thr)
            got = segmented_pass(rows, pos, consumed_end, nf, raw_thr, stats)
            assert np.array_equal(got, full > raw_thr), (g, thr)
            n_pass += int(got.sum())
    assert n_pass > 0
    if name == "rgbd_62":   # the inputs reach both edges of a mid-block test (a one-block row has no mid-block test)
        assert stats["equal"] > 0 and stats["last_one_short"] > 0, stats
    print(name, stats, n_pass)
