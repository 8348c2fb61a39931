"""Where k_score_coarse_sb should test its pruning bound: wave loads per template for several test schedules, on the table model of
sim_score_blocks.py (blocks_of: features -> same-shift triples round robin -> blocks of 5 groups, leftovers padded) and the oracle's
coarsest-level linear memories.  Per 504-placement chunk the model keeps the kernel's per-lane alive flags (63 lanes x 8 placements, a
dead lane is never revived); a chunk stops at the first test no lane survives.  Every processed group costs 3 loads per live chunk,
the padded entries of a leftover group included; the all-padding groups that fill a short LAST block up to five are not charged, though
the kernel loads them too (sim_score_blocks.py's loads_of charges 15 per block) -- few chunks get that far.  The bound at a test after k groups is the kernel's: exact at a block's end, and inside a block the block-end
count of real features minus 3 per group still to come.
Prints the histogram of the group at which a chunk is provably dead (testing after every group), the chunks that survive the tests at
the ends of blocks 1 and 2, and per schedule the loads and bound tests per template.
usage: python scripts/sim_score_schedule.py synth|mesh [threshold] [texture]"""
import sys

import numpy as np

from sim_score_blocks import blocks_of, rows_of, workload

LANES, LANE_POS = 63, 8
MAX_GROUPS = 30
SCHEDULES = {
    "today (5, 10, 15, 20, ...)": [k for k in range(1, MAX_GROUPS + 1) if k % 5 == 0],
    "4, 8, 12, 16, ...": [k for k in range(1, MAX_GROUPS + 1) if k % 4 == 0],
    "5, 7, 9, 12, 15, 20, ...": [5, 7, 9, 12, 15, 20, 25, 30],
    "2 + 2 + 1 (5, 7, 9, 10, 12, 14, 15, ...)": [k for k in range(5, MAX_GROUPS + 1) if k % 5 in (0, 2, 4)],
    "3 + 2 (5, 8, 10, 13, 15, ...)": [k for k in range(5, MAX_GROUPS + 1) if k % 5 in (0, 3)],
    "every group from 5 on": list(range(5, MAX_GROUPS + 1)),
    "every group": list(range(1, MAX_GROUPS + 1)),
}


def chunk_runs(blocks, flat, pos, raw_thr, nf):
    """Per chunk: (group sums [groups, 504] over whole lanes, the kernel's consumed-features bound after each group)"""
    groups = [blk[3 * q:3 * q + 3] for blk in blocks for q in range(len(blk) // 3)]
    pos8 = -(-pos // LANE_POS) * LANE_POS
    rows = np.stack([sum((flat[ft[0]][ft[1]][ft[2]:ft[2] + pos8] for ft in g if ft is not None), np.zeros(pos8, np.int32)) for g in groups])
    real = np.cumsum([sum(ft is not None for ft in g) for g in groups])
    bound = []
    for k in range(1, len(groups) + 1):
        end = min(len(groups), -(-k // 5) * 5)                       # the block's last group (the last block may be short: its slots are padding)
        bound.append(int(real[end - 1]) - 3 * (-(-k // 5) * 5 - k))
    for c0 in range(0, pos, LANES * LANE_POS):
        n8 = min(LANES * LANE_POS, pos8 - c0)
        yield rows[:, c0:c0 + n8].reshape(len(groups), -1, LANE_POS), bound


def run_schedule(sums, bound, tests, raw_thr, nf):
    """-> (groups loaded, tests made) for one chunk; the last group always ends with a test (need = raw_thr + 1)"""
    n_groups = sums.shape[0]
    S = np.zeros(sums.shape[1:], np.int32)
    alive = np.ones(sums.shape[1], bool)
    made = 0
    for k in range(1, n_groups + 1):
        S = S + sums[k - 1]
        if k in tests or k == n_groups:
            need = raw_thr + 1 - 4 * (nf - bound[k - 1])
            if need > 0:
                made += 1
                alive &= (S >= need).any(1)
                if not alive.any():
                    return k, made
    return n_groups, made


def main():
    kind = sys.argv[1] if len(sys.argv) > 1 else "synth"
    thr = float(sys.argv[2]) if len(sys.argv) > 2 else 92.0
    tex = float(sys.argv[3]) if len(sys.argv) > 3 else 0.6
    bank, frames = workload(kind, tex)
    loads = {k: 0 for k in SCHEDULES}
    made = {k: 0 for k in SCHEDULES}
    first_block = 0
    death = np.zeros(MAX_GROUPS + 2, np.int64)     # [MAX_GROUPS + 1]: the chunk holds a passing placement
    survive = [0, 0]
    n = chunks = 0
    for feats, inter, flat, pos, raw_thr, nf, _ in rows_of(bank, frames, thr):
        blocks = blocks_of(inter)
        n += 1
        for sums, bound in chunk_runs(blocks, flat, pos, raw_thr, nf):
            chunks += 1
            for name, tests in SCHEDULES.items():
                g, t = run_schedule(sums, bound, set(tests), raw_thr, nf)
                loads[name] += 3 * g
                made[name] += t
                if name.startswith("today"):
                    first_block += 3 * min(g, 5)
                    survive[0] += g > 5
                    survive[1] += g > 10
            g, _ = run_schedule(sums, bound, set(range(1, MAX_GROUPS + 1)), raw_thr, nf)
            total = sums.sum(0)
            death[MAX_GROUPS + 1 if (total > raw_thr).any() else g] += 1
    print("%s thr %s tex %s: %d templates, %d chunks" % (kind, thr, tex, n, chunks))
    print("  chunks that survive the test after block 1: %.0f %%, after block 2: %.0f %%" % (100 * survive[0] / chunks, 100 * survive[1] / chunks))
    print("  group at which a chunk is provably dead (% of chunks; 'pass' = it holds a passing placement):")
    print("   ", "  ".join("%d: %.1f" % (g, 100 * c / chunks) for g, c in enumerate(death[:MAX_GROUPS + 1]) if c), " pass: %.2f" % (100 * death[-1] / chunks))
    base = loads["today (5, 10, 15, 20, ...)"]
    print("  today's loads per template: %.1f in the first block, %.1f later" % (first_block / n, (base - first_block) / n))
    for name in SCHEDULES:
        print("  tests after groups %-42s loads per template %5.1f (%+5.1f %%)   tests per template %4.1f" % (name, loads[name] / n, 100 * (loads[name] / base - 1), made[name] / n))


if __name__ == "__main__":
    main()
