"""The merged tail pass of k_score_coarse_sb, restated in numpy on top of the model of test_score_schedule_host.py.

A wave scores its template on two frames A and B = A + 8.  When the template's last pass is a one-chunk pass of at most 31 live dwords
(lanes), the two frames' tails share ONE pass: lanes 0..31 work on frame A's tail, lanes 32..63 on frame B's, live flags per lane, the same
`need` for both halves, and the chunk stays on while either half has a live lane.  The two-chunk passes in front stay per frame.

  same candidates   for random group sums, random thresholds and rows of 62, 47, 30 and 17 features, the (frame, template, placement, score)
                    set of the merged schedule is the unmerged one's and the plain full sum's; the plain schedule as restated here is the
                    imported segmented_pass on the same rows
  one half dead     a frame pair where one half dies in block 0 and the other survives to the end, both ways round, and in the surviving
                    half a placement that meets a mid-block test with S == need exactly
  wave loads        a merged pair loads max(A's tail, B's tail) where the plain tails load their sum, so a pair saves min(...) -- at least
                    the 15 loads of block 0 -- and on a bank with three-chunk templates (oracle memories of two scenes) the modelled loads
                    per template and frame fall by exactly that, which is at least 7.5 x the share of templates with a mergeable tail"""
import numpy as np
import pytest

import np_restatement as R
import test_score_schedule_host as T
from linemod_pose_estimation_amd import synth
from oracle import oracle as o

CHUNK_LANES, LANE_POS = T.CHUNK_LANES, T.LANE_POS
CHUNK_POS = CHUNK_LANES * LANE_POS
HALF_LANES, TAIL_LANES = 32, 31          # lanes of a half-wave; live dwords a merged tail holds at the most (lanes 31 and 63 own nothing)


def segments_of(b):
    return [(0, R.SB_GROUPS)] if b == 0 else list(zip(np.cumsum((0,) + T.SEGMENTS[:-1]).tolist(), T.SEGMENTS))


def chunk_pass(sums, real, consumed_end, nf, raw_thr, stats=None):
    """One chunk of any lane count.  sums [groups, lanes * 8]: the group sums of the lanes' placements; real [lanes * 8]: the placement
    exists.  -> (boolean [lanes * 8] of the placements appended, wave loads issued).  A lane starts alive if its first placement exists."""
    lanes = real.size // LANE_POS
    real2 = real.reshape(lanes, LANE_POS)
    alive = real2[:, 0].copy()
    S = np.zeros(real.size, np.int64)
    loads = 0
    if not alive.any():
        return np.zeros(real.size, bool), 0
    for b, end in enumerate(consumed_end):
        for g0, ng in segments_of(b):
            loads += 3 * ng
            S += sums[5 * b + g0:5 * b + g0 + ng].sum(0)
            need = raw_thr + 1 - 4 * (nf - (end - 3 * (R.SB_GROUPS - g0 - ng)))
            if need <= 0:
                continue
            S2 = S.reshape(lanes, LANE_POS)
            if stats is not None and b > 0 and g0 + ng < R.SB_GROUPS:
                stats["equal"] += int(((S2 == need) & alive[:, None] & real2).sum())
            alive &= (S2 >= need).any(1)
            if not alive.any():
                if stats is not None:
                    stats["died_in_block"].append(b)
                return np.zeros(real.size, bool), loads
    return np.repeat(alive, LANE_POS) & real & (S > raw_thr), loads


def padded(rows, c0, n):
    out = np.zeros((rows.shape[0], n), np.int64)
    m = max(0, min(n, rows.shape[1] - c0))
    out[:, :m] = rows[:, c0:c0 + m]
    return out


def plain_chunk(rows, pos, c0, consumed_end, nf, raw_thr, stats=None):
    return chunk_pass(padded(rows, c0, CHUNK_POS), np.arange(CHUNK_POS) < pos - c0, consumed_end, nf, raw_thr, stats)


def tail_start(pos):
    """First placement of the template's one-chunk pass, or None when its last pass is a two-chunk pass."""
    n_chunks = -(-pos // CHUNK_POS)
    return (n_chunks - 1) * CHUNK_POS if n_chunks % 2 else None


def mergeable(pos):
    c0 = tail_start(pos)
    return c0 is not None and -(-(pos - c0) // LANE_POS) <= TAIL_LANES


def schedule(rows_a, rows_b, pos, consumed_end, nf, raw_thr, merge, stats=None):
    """A wave's two frames -> (passing [2, pos], wave loads of the pair, wave loads of the tail passes alone)."""
    passing = np.zeros((2, pos), bool)
    loads = tail_loads = 0
    merged = merge and mergeable(pos)
    c_tail = tail_start(pos)
    for f, rows in enumerate((rows_a, rows_b)):
        for c0 in range(0, pos, CHUNK_POS):
            if merged and c0 == c_tail:
                continue
            got, n = plain_chunk(rows, pos, c0, consumed_end, nf, raw_thr)
            passing[f, c0:c0 + CHUNK_POS] = got[:pos - c0]
            loads += n
            tail_loads += n if c0 == c_tail else 0
    if merged:
        half = HALF_LANES * LANE_POS
        sums = np.concatenate([padded(rows_a, c_tail, half), padded(rows_b, c_tail, half)], 1)
        real = np.tile(np.arange(half) < pos - c_tail, 2)
        assert not real.reshape(2, HALF_LANES, LANE_POS)[:, TAIL_LANES].any()      # lanes 31 and 63 own no placement
        got, n = chunk_pass(sums, real, consumed_end, nf, raw_thr, stats)
        passing[0, c_tail:] = got[:pos - c_tail]
        passing[1, c_tail:] = got[half:half + pos - c_tail]
        loads += n
        tail_loads += n
    return passing, loads, tail_loads


def candidates(passing, rows_a, rows_b, pos, template):
    full = (rows_a[:, :pos].sum(0), rows_b[:, :pos].sum(0))
    return {(f, template, int(j), int(full[f][j])) for f in (0, 1) for j in np.flatnonzero(passing[f])}


def blocks_of(nf):
    """consumed_end per block and groups of a row of nf real features without padding in front of its last group."""
    n_groups = -(-nf // 3)
    n_blocks = -(-n_groups // R.SB_GROUPS)
    return [min(nf, 15 * (b + 1)) for b in range(n_blocks)], n_groups, n_blocks


def random_rows(rng, nf, pos, hot):
    """Group sums [5 * blocks, pos rounded up to lanes]: a quiet background (0..2 per feature) with `hot` placements near the maximum."""
    consumed_end, n_groups, n_blocks = blocks_of(nf)
    pos8 = -(-pos // LANE_POS) * LANE_POS
    per_group = np.array([3] * (nf // 3) + ([nf % 3] if nf % 3 else []))
    rows = np.zeros((R.SB_GROUPS * n_blocks, pos8), np.int64)
    rows[:n_groups] = rng.integers(0, 3, (n_groups, pos8)) * per_group[:, None]
    for j in rng.integers(0, pos, hot):
        rows[:n_groups, j] = np.minimum(4 * per_group, rng.integers(2, 5, n_groups) * per_group + rng.integers(0, 2, n_groups))
    assert (rows[:n_groups] <= 4 * per_group[:, None]).all()
    return rows, consumed_end


@pytest.mark.parametrize("nf", (62, 47, 30, 17))
def test_merged_schedule_appends_the_unmerged_candidates(nf):
    rng = np.random.default_rng(20261020 + nf)
    # 150 dwords as at 640x480 (tails of 1, 8, 19 and 24 lanes), the largest and the first unmergeable tail, one chunk, two chunks
    shapes = [1009, 1065, 1160, 1200, 1256, 1257, 1008 + 504, 8, 248, 249, 504, 1008, 2016 + 100]
    n_pass = n_merged = 0
    for template, pos in enumerate(shapes):
        rows_a, consumed_end = random_rows(rng, nf, pos, hot=int(rng.integers(0, 6)))
        rows_b, _ = random_rows(rng, nf, pos, hot=int(rng.integers(0, 6)))
        for thr in (50, 62, 74, 86, 98):
            raw_thr = T.raw_threshold(nf, thr)
            plain, loads_plain, tail_plain = schedule(rows_a, rows_b, pos, consumed_end, nf, raw_thr, merge=False)
            for f, rows in enumerate((rows_a, rows_b)):     # the restatement of the plain schedule is the imported model's
                assert np.array_equal(plain[f], T.segmented_pass(rows, pos, consumed_end, nf, raw_thr, {"equal": 0, "last_one_short": 0}))
                assert np.array_equal(plain[f], rows[:, :pos].sum(0) > raw_thr)
            merged, loads_merged, tail_merged = schedule(rows_a, rows_b, pos, consumed_end, nf, raw_thr, merge=True)
            assert candidates(merged, rows_a, rows_b, pos, template) == candidates(plain, rows_a, rows_b, pos, template), (pos, thr)
            if mergeable(pos):
                n_merged += 1
                assert loads_plain - loads_merged == tail_plain - tail_merged >= 15
            else:
                assert loads_merged == loads_plain
            n_pass += int(merged.sum())
    assert [mergeable(p) for p in shapes] == [True] * 5 + [False] * 2 + [True] * 2 + [False] * 3 + [True]
    assert n_pass > 0 and n_merged > 0


def planted_rows(nf, pos, j_star, sums_star):
    consumed_end, n_groups, n_blocks = blocks_of(nf)
    rows = np.zeros((R.SB_GROUPS * n_blocks, -(-pos // LANE_POS) * LANE_POS), np.int64)
    if j_star is not None:
        rows[:n_groups, j_star] = sums_star
    return rows, consumed_end


@pytest.mark.parametrize("survivor", (0, 1))
def test_one_half_dies_in_block_0_and_the_other_survives_with_s_equal_need(survivor):
    nf, thr, pos = 62, 80, 1200
    raw_thr = T.raw_threshold(nf, thr)
    assert raw_thr == 223
    # the surviving placement: every feature at 4 but groups 5 and 6 empty, so that the test behind group 7 (block 1, 3 of 5 groups:
    # consumed >= 30 - 6 = 24, need = 224 - 4 * 38 = 72) sees S = 6 * 12 = 72 == need; it ends with 18 * 12 + 8 = 224 > 223
    sums_star = np.array([12] * 5 + [0, 0] + [12] * 13 + [8])
    assert T.SEGMENTS[0] == 3 and sums_star.sum() == raw_thr + 1
    j_star = 1008 + 8 * 23 + 5       # the tail's last live lane
    busy, consumed_end = planted_rows(nf, pos, j_star, sums_star)
    blank, _ = planted_rows(nf, pos, None, None)
    rows = (busy, blank) if survivor == 0 else (blank, busy)
    stats = {"equal": 0, "died_in_block": []}
    merged, loads, tail_loads = schedule(rows[0], rows[1], pos, consumed_end, nf, raw_thr, merge=True, stats=stats)
    # the pair ran to the end, the dead half riding along; behind the first S == need every feature adds its 4 and `need` rises by as much,
    # so the mid-block tests of blocks 1, 2 and 3 all see equality (block 4's comes behind the row's last real feature)
    assert stats["equal"] == 3 and stats["died_in_block"] == []
    assert candidates(merged, rows[0], rows[1], pos, 0) == {(survivor, 0, j_star, raw_thr + 1)}
    # alone, the blank frame's tail dies in block 0 and the busy one's runs all five blocks
    for f in (0, 1):
        st = {"equal": 0, "died_in_block": []}
        got, n = plain_chunk(rows[f], pos, 1008, consumed_end, nf, raw_thr, st)
        assert (st["died_in_block"], n, int(got.sum())) == (([], 75, 1) if f == survivor else ([0], 15, 0))
    assert tail_loads == 75
    plain, loads_plain, _ = schedule(rows[0], rows[1], pos, consumed_end, nf, raw_thr, merge=False)
    assert np.array_equal(plain, merged) and loads_plain - loads == 15
    # one below the bound at the same test: the whole pair stops there
    sums_low = sums_star.copy()
    sums_low[7] = 11
    low, _ = planted_rows(nf, pos, j_star, sums_low)
    st = {"equal": 0, "died_in_block": []}
    merged, _, _ = schedule(low, blank, pos, consumed_end, nf, raw_thr, merge=True, stats=st)
    assert st["died_in_block"] == [1] and not merged.any()


def test_modelled_wave_loads_fall_by_the_predicted_amount():
    W, H, thr = T.W, T.H, 86
    bank = synth.make_bank(24, T=(5, 8), seed=20261021, num_features=63, size_range=(30.0, 110.0))
    t = T.rows_of(bank)
    L, M = len(bank.T), len(bank.modalities)
    cells = int(t["geom"]["cells"])
    od = o.OracleDetector(bank)
    flats = []
    for seed in (8101, 8102):
        sources, _ = synth.make_scene(bank, W, H, seed=seed)
        od.match(sources, 90.0)
        flats.append([np.concatenate([od.linear_memory(L - 1, m, (H >> (L - 1), W >> (L - 1))).astype(np.int32).reshape(8, -1),
                                      np.zeros((8, cells + 8 * CHUNK_POS), np.int32)], 1) for m in range(M)])
    n_g = len(t["blk"])
    positions = t["sinfo"][:, 0]
    three = np.array([-(-int(p) // CHUNK_POS) == 3 for p in positions])
    can = np.array([mergeable(int(p)) for p in positions])
    assert three.sum() >= 4 and (can == three).all()       # 150 dwords: every third chunk has at most 24 lanes
    plain_total = merged_total = predicted_saving = first_block_saving = 0
    n_pass = 0
    for g in range(n_g):
        rows_a, consumed_end = T.group_rows(t, g, flats[0], cells)
        rows_b, _ = T.group_rows(t, g, flats[1], cells)
        nf, pos = int(t["sinfo"][g, 1]), int(positions[g])
        raw_thr = T.raw_threshold(nf, thr)
        plain, loads_plain, _ = schedule(rows_a, rows_b, pos, consumed_end, nf, raw_thr, merge=False)
        merged, loads_merged, _ = schedule(rows_a, rows_b, pos, consumed_end, nf, raw_thr, merge=True)
        assert candidates(merged, rows_a, rows_b, pos, g) == candidates(plain, rows_a, rows_b, pos, g)
        assert np.array_equal(merged[0], rows_a[:, :pos].sum(0) > raw_thr) and np.array_equal(merged[1], rows_b[:, :pos].sum(0) > raw_thr)
        n_pass += int(merged.sum())
        plain_total += loads_plain
        merged_total += loads_merged
        if can[g]:
            c0 = tail_start(pos)
            tails = [plain_chunk(rows, pos, c0, consumed_end, nf, raw_thr)[1] for rows in (rows_a, rows_b)]
            predicted_saving += min(tails)
            first_block_saving += 15
    per = 1.0 / (2 * n_g)       # per template and frame
    print("wave loads per template and frame: plain %.2f merged %.2f; three-chunk share %.3f; saving %.2f (block 0 alone %.2f)"
          % (plain_total * per, merged_total * per, three.mean(), predicted_saving * per, first_block_saving * per))
    assert n_pass > 0
    assert plain_total - merged_total == predicted_saving >= first_block_saving
    assert first_block_saving * per == pytest.approx(7.5 * can.mean())
