"""The label seam and the families of tests/label_cases.py, checked on the CPU.

  the seam      for synth scenes, the oracle's match_labels on its own label images returns what match returned on the sources (matches, raw
                records, candidates), and the numpy restatement's match_labels equals the oracle's on every family
  the claims    whatever a family says it reaches is asserted from the reference alone: the 8 x 256 coverage of both response tables, the
                placements with raw == raw_threshold and raw_threshold + 1, S == need at a bound test (the CPU model of the segmented pass in
                test_score_schedule_host.py), ties that tie, sums of 252 M, every P placement the template's best
  the mutants   deliberately wrong variants of the restatement each disagree with the oracle on a case of the family meant for them

`reference` (the oracle's matches per frame of a case, computed once, never modified) also serves tests/test_gpu_label_match.py."""
import numpy as np
import pytest

import label_cases as lc
import np_restatement as R
import test_score_schedule_host as host
from linemod_pose_estimation_amd import synth
from oracle import oracle as o

F32 = np.float32
# tight instances; those whose row has more than one block; those whose planted placement has S == need at a MID-block test (the others meet
# equality at block-end tests only: the blocks behind their lowered features hold padding, which keeps the mid-block count a lower bound)
TIGHT_COUNTS = (52, 44, 16)
_ods, _refs = {}, {}


def oracle_of(bank):
    if id(bank) not in _ods:
        _ods[id(bank)] = (bank, o.OracleDetector(bank))
    return _ods[id(bank)][1]


def as_set(m):
    return sorted(zip(*(m[k].tolist() for k in ("x", "y", "similarity", "template_id", "class_index"))))


def visits(case):
    """[(threshold, class ids)] of the oracle calls that make up the case's call: one, or one per class of a per-class mapping."""
    if isinstance(case.threshold, dict):
        order = case.class_ids or sorted(case.threshold, key=lambda s: s.encode())
        return [(float(case.threshold[c]), (c,)) for c in order if c in case.threshold]
    return [(float(case.threshold), case.class_ids)]


def reference(case, f):
    """-> (matches of frame f as a sorted list, coarse candidates, raw records as a sorted list); computed once per (bank, frame, call)."""
    key = (id(case.bank), id(case.frames[f]), repr(case.threshold), case.class_ids)
    if key not in _refs:
        od = oracle_of(case.bank)
        matches, raw, cands = [], [], 0
        for thr, cids in visits(case):
            matches += as_set(od.match_labels(case.frames[f], thr, class_ids=cids))
            raw += as_set(od.last_raw())
            cands += od.last_candidates()
        _refs[key] = (sorted(matches), cands, sorted(raw), case.frames[f])   # the frame is kept: its id stays its own
    return _refs[key][:3]


def restated(case, f, **kw):
    """The numpy restatement's raw records of frame f as a sorted list, and its candidates."""
    names = sorted(c[0] for c in case.bank.classes)
    stats = {}
    rec = R.match_labels(case.bank, case.frames[f], case.threshold, class_ids=case.class_ids, stats=stats, **kw)
    return sorted((x, y, float(s), tid, names.index(cid)) for x, y, s, cid, tid in rec), stats["candidates"]


def coarse_memories(case, f):
    """The oracle's coarsest-level linear memories [modality] of frame f (after reference(case, f))."""
    od = oracle_of(case.bank)
    L, M = len(case.bank.T), len(case.bank.modalities)
    thr, cids = visits(case)[0]
    od.match_labels(case.frames[f], thr, class_ids=cids)
    return [od.linear_memory(L - 1, m, (case.H >> (L - 1), case.W >> (L - 1))) for m in range(M)]


def coarse_totals(case, lms, cid, tid):
    """Sum over the modalities of similarity() of template (cid, tid) on the coarsest level -> (int array [Hc, Wc], positions, nf)."""
    L, M = len(case.bank.T), len(case.bank.modalities)
    tpl = lc.template_of(case.bank, cid, tid)
    size = (case.W >> (L - 1), case.H >> (L - 1))
    tot, nf, pos = 0, 0, None
    for m in range(M):
        w, h, f = tpl[L - 1][m]
        s, pos = R.similarity(lms[m], size, case.bank.T[-1], (w, h), [tuple(v) for v in f.tolist()])
        tot = tot + s.astype(np.int64)
        nf += len(f)
    return tot, pos, nf


# ---- the seam --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mods,T,W,H", [((lc.CG, lc.DN), (5, 8), 320, 240), ((lc.DN, lc.CG), (4, 8), 256, 192), ((lc.CG,), (4, 8, 10), 320, 320)])
def test_match_labels_on_the_oracles_own_labels_is_match(mods, T, W, H):
    bank = synth.make_bank(10, modalities=mods, T=T, seed=31, size_range=(24.0, 60.0))
    sources, _ = synth.make_scene(bank, W, H, seed=32)
    od = o.OracleDetector(bank)
    want = od.match(sources, 75.0)
    raw, cands = od.last_raw(), od.last_candidates()
    L, M = len(T), len(mods)
    labels = [[od.quantized(l, m, (H >> l, W >> l)) for m in range(M)] for l in range(L)]
    lms = [[od.linear_memory(l, m, (H >> l, W >> l)) for m in range(M)] for l in range(L)]
    got = od.match_labels(labels, 75.0)
    assert len(want) > 0 and np.array_equal(got, want) and np.array_equal(od.last_raw(), raw) and od.last_candidates() == cands > 0
    for l in range(L):
        for m in range(M):
            assert np.array_equal(od.quantized(l, m, (H >> l, W >> l)), labels[l][m])
            assert np.array_equal(od.linear_memory(l, m, (H >> l, W >> l)), lms[l][m])
    if len(T) == 2 and W == 320:   # the restatement's two halves against the oracle's, on a scene
        assert [[np.array_equal(a, b) for a, b in zip(x, y)] for x, y in zip(R.quantize_pyramid(bank, sources), labels)] == [[True] * M] * L
    with pytest.raises(ValueError):
        od.match_labels([labels[0]], 75.0)


@pytest.mark.parametrize("name", list(lc.FAMILIES))
def test_restatement_equals_the_oracle_on_every_family(name):
    n = 0
    for case in lc.family(name):
        seen = set()
        for f in range(len(case.frames)):
            if id(case.frames[f]) in seen:
                continue
            seen.add(id(case.frames[f]))
            _, cands, raw = reference(case, f)
            got, got_cands = restated(case, f)
            assert got == raw and got_cands == cands, (case.name, f)
            n += len(raw)
    assert n > 0


# ---- the claims ------------------------------------------------------------------------------------------------------------------------
def test_r_coarse_every_byte_at_every_nibble_position():
    for case in lc.family("r_coarse"):
        c = case.claims[0]
        seen = [set() for _ in range(8)]
        for lab in case.frames:
            spr = o.spread(lab[1][0], c["T"])
            assert np.array_equal(spr, R.spread(lab[1][0], c["T"]))
            anchors = spr[::c["T"], ::c["T"]].reshape(-1)
            assert len(anchors) == c["Wc"] * c["Hc"]
            for idx, v in enumerate(anchors.tolist()):
                seen[idx % 8].add(v)
        assert all(s == set(range(256)) for s in seen), case.name


def test_r_fine_every_orientation_meets_every_byte():
    for case in lc.family("r_fine"):
        c = case.claims[0]
        window = {(v, kind): (f, cx, cy) for f, cx, cy, v, kind in c["where"]}
        assert len(window) == len(c["where"]) == 256 * (1 if c["variant"] == "plain" else len(lc.NEIGHBOURS))
        for f, cx, cy, v, kind in c["where"]:
            assert o.spread(case.frames[f][0][0], 5)[5 * cy, 5 * cx] == v
            if kind:
                assert {int(o.spread(case.frames[f][0][0], 5)[5 * cy, 5 * (cx + d)]) for d in (-3, -2, -1, 1, 2, 3)} == {lc.neighbour_byte(kind, v)}
        # the triples the case is for, from the rule alone; each is looked up in the raw records (std::unique compares position, similarity
        # and class only, so another template's equal match may absorb one in the final list)
        assert sorted(c["expect"]) == sorted(lc.r_fine_expectations(c["variant"])) and len(set(c["expect"])) == len(c["expect"])
        for orient, v, kind, r in c["expect"]:
            f, cx, cy = window[v, kind]
            got = {m[2] for m in reference(case, f)[2] if (m[0], m[1], m[3]) == (5 * cx + 2, 5 * cy + 2, orient)}
            assert got == ({25.0 * r} if r else set()), (case.name, f, v, kind, orient)
        if c["variant"] == "plain":
            assert {(oo, v) for oo, v, _, _ in c["expect"]} == {(oo, v) for oo in range(8) for v in range(256)}      # complete, not sampled
        else:
            # how many (orientation, byte) pairs have each neighbour byte strictly below the target, and for which orientations: 0x7f
            # answers 4 to orientations 0..6 and 3 to orientation 7, so it lies below the 128 targets with bit 7 for orientation 7 alone;
            # 0x80 answers 4 to orientation 7
            count = {k: sum(kind == k for _, _, kind, _ in c["expect"]) for k in lc.NEIGHBOURS}
            assert count == {"0x00": 2010, "0x7f": 128, "0x80": 1594, "0xfe_without_target": 1088}
            reach = {k: {oo for oo, _, kind, _ in c["expect"] if kind == k} for k in lc.NEIGHBOURS}
            assert reach == {"0x00": set(range(8)), "0x7f": {7}, "0x80": set(range(7)), "0xfe_without_target": set(range(8))}


def test_r_fine_three_levels_reads_the_response_at_level_1():
    seen = set()
    for case in lc.family("r_fine_levels3"):
        xy = case.claims[0]["xy"]
        for v in range(256):
            assert o.spread(case.frames[v][1][0], 8)[64, 64] == v
            raw = reference(case, v)[2]
            n_cand = reference(case, v)[1]
            assert 8 * 4 <= n_cand == reference(case, 0)[1]            # at least the four tiled placements per template, whatever the byte
            for orient in range(8):
                r = lc.response_of(orient, v)
                here = [m for m in raw if m[3] == orient]
                assert all((m[0], m[1], m[2]) == (xy[0], xy[1], 100.0) for m in here) and (len(here) >= 4) == (25.0 * r >= case.threshold) == (len(here) > 0), (case.name, v, orient)
                seen.add((orient, v))
    assert len(seen) == 8 * 256
    # the four thresholds separate the five responses
    assert [sum(25.0 * r >= t for t in lc.R_FINE3_THRESHOLDS) for r in range(5)] == [0, 1, 2, 3, 4]


def sum_claims(names):
    for name in names:
        for case in lc.family(name):
            by_frame = {}
            for c in case.claims:
                if c["kind"] == "coarse_sum":
                    by_frame.setdefault(c["frame"], []).append(c)
            for f, claims in by_frame.items():
                yield case, f, claims


def test_equality_placements_exist():
    n_edge = n_cand = 0
    for case, f, claims in sum_claims(("s_thresholds", "s_tight", "per_class", "f_depth")):
        lms = coarse_memories(case, f)
        Wc = (case.W >> (len(case.bank.T) - 1)) // case.bank.T[-1]
        for c in claims:
            cid = c.get("cls", case.bank.classes[0][0])
            tot, pos, nf = coarse_totals(case, lms, cid, c["template"])
            thr = case.threshold[cid] if isinstance(case.threshold, dict) else case.threshold
            assert c["raw_threshold"] == o.raw_threshold(nf, thr) == R.raw_threshold(nf, thr)
            cx, cy = c["cell"]
            assert cy * Wc + cx < pos and tot[cy, cx] == c["total"], (case.name, f, c, int(tot[cy, cx]))
            assert c["candidate"] == (c["total"] == c["raw_threshold"] + 1) and (c["candidate"] or c["total"] == c["raw_threshold"])
            n_edge += not c["candidate"]
            n_cand += c["candidate"]
    assert n_edge > 300 and n_cand > 250, (n_edge, n_cand)      # fewer candidates: raw_threshold + 1 > 4 nf has no instance


def tight_rows(case, f, template):
    """-> (the model's rows [groups, positions], consumed_end per block, positions, nf, real features per group) of a template on frame f."""
    t = host.rows_of(case.bank, case.W, case.H)
    L, M = len(case.bank.T), len(case.bank.modalities)
    cells = int(t["geom"]["cells"])
    lms = coarse_memories(case, f)
    flat = [np.concatenate([lms[m].astype(np.int32).reshape(8, -1), np.zeros((8, cells + 8 * lc.CHUNK_POS), np.int32)], 1) for m in range(M)]
    rows, consumed_end = host.group_rows(t, template, flat, cells)
    zero_byte = int(t["geom"]["nib_zero_off"]) // 4 * 4
    real = [int(sum(int(off) % t["uni_block"] != zero_byte for off in t["blk"][template, b, 3 * q:3 * q + 3]))
            for b in range(len(consumed_end)) for q in range(R.SB_GROUPS)]
    return rows, consumed_end, int(t["sinfo"][template, 0]), int(t["sinfo"][template, 1]), real


def bound_tests(consumed_end):
    """The model's bound tests in order: (block, groups consumed so far, the kernel's count of features consumed, mid-block?)."""
    for b, end in enumerate(consumed_end):
        for g0, ng in ([(0, R.SB_GROUPS)] if b == 0 else zip(np.cumsum((0,) + host.SEGMENTS[:-1]), host.SEGMENTS)):
            yield b, R.SB_GROUPS * b + int(g0) + ng, end - 3 * (R.SB_GROUPS - int(g0) - ng), b > 0 and int(g0) + ng < R.SB_GROUPS


def test_tight_bound_instances_meet_the_bound_with_equality_and_a_stricter_bound_loses_them():
    """Every instance marked tight, one by one.  Its missing response sits in the features the table serves first, so at every bound test
    that comes behind those features and whose count of consumed features is the true one (every block-end test; a mid-block test when the
    rest of its block holds no padding) the planted placement has S == need exactly; where the count is a lower bound, S > need.  With need
    + 1 every instance loses its candidate; with the shipped bound none does."""
    checked = multi_block = mid_equal = 0
    Wc = (lc.S_W >> 1) // lc.S_T[1]
    for case, f, claims in sum_claims(("s_tight",)):
        for c in claims:
            if not c["tight"]:
                continue
            rows, consumed_end, pos, nf, real = tight_rows(case, f, c["template"])
            p = c["cell"][1] * Wc + c["cell"][0]
            rt = c["raw_threshold"]
            lowered_features = -(-(4 * nf - (rt + 1)) // 4)
            assert sum(real) == nf == consumed_end[-1] and rows[:, p].sum() == rt + 1
            exact = mid = 0
            for b, groups, counted, is_mid in bound_tests(consumed_end):
                need = rt + 1 - 4 * (nf - counted)
                true_count = sum(real[:groups])
                assert counted <= true_count
                if need <= 0:
                    continue
                S = int(rows[:groups, p].sum())
                if counted == true_count and lowered_features <= true_count:
                    assert S == need, (case.name, f, nf, b, groups, S, need)
                    exact += 1
                    mid += is_mid
                else:
                    assert S >= need, (case.name, f, nf, b, groups, S, need)
            assert exact >= 1, (case.name, f, nf)
            full = rows[:, :pos].sum(0)
            got = host.segmented_pass(rows, pos, consumed_end, nf, rt, {"equal": 0, "last_one_short": 0})
            assert np.array_equal(got, full > rt) and got[p], (case.name, f)                 # the shipped bound loses none
            strict = host.segmented_pass(rows, pos, consumed_end, nf, rt, {"equal": 0, "last_one_short": 0}, need_offset=1)
            assert not strict[p], (case.name, f, nf)                                       # one too strict: the planted candidate is lost
            checked += 1
            multi_block += len(consumed_end) > 1
            mid_equal += mid > 0
    print("tight instances", checked, "with more than one block", multi_block, "with S == need at a mid-block test", mid_equal)
    assert (checked, multi_block, mid_equal) == TIGHT_COUNTS


def test_saturated_sums():
    for case in lc.family("saturated"):
        M = case.claims[0]["M"]
        lms = coarse_memories(case, 0)
        n = 0
        for tid in range(case.bank.num_templates()):
            tpl = lc.template_of(case.bank, "sat", tid)
            for m in range(M):
                w, h, f = tpl[1][m]
                s, pos = R.similarity(lms[m], (case.W >> 1, case.H >> 1), 8, (w, h), [tuple(v) for v in f.tolist()])
                assert (s.reshape(-1)[:pos] == 252).all()
            tot, pos, nf = coarse_totals(case, lms, "sat", tid)
            assert nf == 63 * M and (tot.reshape(-1)[:pos] == 252 * M).all()
            n += pos
        assert reference(case, 0)[1] == n > 16 * 256        # every placement is a candidate: more than 16 per workgroup of any grid up to 256
        assert all(m[2] == 100.0 for m in reference(case, 0)[0])


def test_p_placements_are_the_templates_best():
    for T, W, H in lc.P_SETS.values():
        targets, npos, (Wc, Hc) = lc.p_targets(T, W, H)
        assert {0, 7, 8, 503, 504, 1007, 1008, npos[0] - 1} <= set(targets[0]) and {1008, npos[1] - 1} <= set(targets[1])
        tail = npos[0] - 1008
        if W == 704:
            assert -(-tail // 8) == 39 and {1008 + 8 * 30, 1008 + 8 * 31, 1008 + 8 * 32} <= set(targets[0])
        else:
            assert -(-tail // 8) == 24 and npos[1] == 1009          # 24 live lanes; the wide template's tail is one placement
    shifts = set()
    for case in lc.family("p"):
        f = case.instance_frame
        lms = coarse_memories(case, f)
        g = dict(T=8, Wc=(case.W >> 1) // 8, cells=(case.W >> 1) // 8 * ((case.H >> 1) // 8))
        for c in case.claims:
            tot, pos, nf = coarse_totals(case, lms, "p", c["template"])
            flat = tot.reshape(-1)[:pos]
            assert pos == c["positions"] and flat[c["placement"]] == 4 * nf == flat.max(), (case.name, c)
            shifts |= {int(R.linear_index(g, x, y) + c["placement"]) & 7 for x, y, _ in lc.template_of(case.bank, "p", c["template"])[1][0][2].tolist()}
        zero = [i for i in range(len(case.frames)) if i != f]
        assert all(reference(case, i)[:2] == ([], 0) for i in zero[:1])
        raw = reference(case, f)[2]
        # the instance is found (two templates share their level-0 features, so a patch may hold both instances: the first one wins)
        assert all(any(m[2] == 100.0 and m[3] == c["template"] and abs(m[0] - c["xy"][0]) <= 40 and abs(m[1] - c["xy"][1]) <= 40 for m in raw) for c in case.claims)
    assert shifts == set(range(8))


def test_f_claims():
    n = 0
    for name in ("f_wave_split", "f_argmax", "f_equality", "f_depth"):
        for case in lc.family(name):
            thr = case.threshold
            for c in case.claims:
                got = reference(case, c["frame"])[2]
                here = [m for m in got if (m[0], m[1]) == tuple(c.get("xy", ())) and m[3] == c["template"]]
                if c["kind"] == "match":
                    assert [m[2] for m in here] == [float(F32(F32(c["best"]) * F32(100.0) / F32(4 * c["nf"])))], (case.name, c, got[:4])
                elif c["kind"] == "refine_edge":
                    assert [m[2] for m in here] == ([c["sim"]] if c["kept"] else []), (case.name, c)
                    assert reference(case, c["frame"])[1] >= 1
                elif c["kind"] == "best_zero":
                    assert [m[2] for m in here] == ([0.0] if thr == 0.0 else []), (case.name, c)
                elif c["kind"] == "tie":
                    od = oracle_of(case.bank)
                    od.match_labels(case.frames[c["frame"]], thr)
                    lms = [od.linear_memory(0, m, (case.H, case.W)) for m in range(2)]
                    tpl = lc.template_of(case.bank, "f", 0)
                    x1, y1 = (v * lc.F_T[1] + lc.offset_of(lc.F_T[1]) for v in c["coarse_cell"])
                    ocx, ocy = lc.patch_origin(case.bank, case.W, case.H, tpl, 0, x1, y1)
                    patch = sum(R._local_sums(lms[m].reshape(8, -1), (case.W // 5) * (case.H // 5), case.W // 5, (case.W, case.H), 5,
                                              [tuple(v) for v in tpl[0][m][2].tolist()], (ocx + 8) * 5, (ocy + 8) * 5) for m in range(2))
                    ys, xs = np.nonzero(patch == patch.max())
                    assert patch.max() == c["best"] and sorted(zip(xs.tolist(), ys.tolist())) == sorted(c["cells"]), (case.name, c)
                    assert (xs[0], ys[0]) == c["first"] and {m[2] for m in here} == {100.0}
                n += 1
    assert n > 80


def test_f_clamps_reach_every_clamp():
    case = lc.family("f_clamps")[0]
    T, border = 5, 40
    sides = set()
    for tid in range(4):
        tpl = lc.template_of(case.bank, "f", tid)
        w, h, feats = tpl[0][0]
        max_x, max_y = case.W - w - border, case.H - h - border
        raw = [2 * (8 * c + 3) + 1 for c in range(20)]
        assert min(raw) < border and max(raw) > max(max_x, 0)             # both clamps of x act on some candidate
        for x in {min(max(v, border), max_x) for v in raw}:
            for y in {min(max(2 * (8 * r + 3) + 1, border), max_y) for r in range(15)}:
                ox, oy = (int(x / T) - 8) * T, (int(y / T) - 8) * T
                for fx, fy, _ in feats.tolist():
                    sides |= {s for s, out in (("left", fx + ox < 0), ("top", fy + oy < 0), ("right", fx + ox >= case.W), ("bottom", fy + oy >= case.H)) if out}
        if tid in (1, 3):
            assert max_x < border and int(max_x / T) - 8 < 0
    assert sides == {"left", "top", "right", "bottom"}
    assert all(len(reference(case, f)[0]) > 50 for f in range(2))


# ---- do the tests bite? ----------------------------------------------------------------------------------------------------------------
def disagreements(family, **kw):
    n = 0
    for case in lc.family(family):
        for f in range(len(case.frames)):
            _, cands, raw = reference(case, f)
            got, got_cands = restated(case, f, **kw)
            n += (got != raw) or (got_cands != cands)
    return n


def test_mutant_ge_at_the_coarse_test():
    assert disagreements("per_class", mutant="coarse_ge") >= 2 and disagreements("f_depth", mutant="coarse_ge") >= 1
    case = lc.family("s_thresholds")[1]
    assert sum(restated(case, f, mutant="coarse_ge")[1] != reference(case, f)[1] for f in range(len(case.frames))) == len(case.frames)


def test_mutant_last_maximum():
    assert disagreements("f_argmax", mutant="last_max") >= 8


def test_mutant_le_at_the_refinement_test():
    cases = [c for c in lc.family("f_equality") if c.name.endswith("_at")]
    n = sum(restated(c, 0, mutant="refine_le")[0] != reference(c, 0)[2] for c in cases)
    assert n >= 8, n


def test_mutant_u8_wrap_of_the_saturated_sum():
    for case in lc.family("saturated")[1:]:        # M = 2, 3: 504 and 756 do not fit a byte
        assert restated(case, 0, mutant="u8_wrap")[1] != reference(case, 0)[1]


@pytest.mark.parametrize("orient", range(8))
@pytest.mark.parametrize("high", (0, 1))
def test_mutant_response_table_entry_off_by_one(orient, high):
    """One entry of the 8 x 256 table (orientation, nibble side, nibble 1 << orient % 4 or its neighbour) raised or lowered by one: the
    coarse family's linear memories and the fine family's matches both notice."""
    nib = 1 << (orient % 4)
    lut = R.similarity_lut_from_rule().copy()
    e = 32 * orient + 16 * high + nib
    lut[e] = lut[e] - 1 if lut[e] else 1
    case = lc.family("r_coarse")[0]
    od = oracle_of(case.bank)
    differ = 0
    for lab in case.frames:
        od.match_labels(lab, 90.0)
        mem = od.linear_memory(1, 0, (case.H >> 1, case.W >> 1))
        good = np.stack([R.linearize(r, 8) for r in R.response_maps(R.spread(lab[1][0], 8))])
        bad = np.stack([R.linearize(r, 8) for r in R.response_maps(R.spread(lab[1][0], 8), lut)])
        assert np.array_equal(mem, good)
        differ += not np.array_equal(mem, bad)
    assert differ > 0
    case = lc.family("r_fine")[0]
    v = nib << (4 * high)
    f = next(fr for fr, _, _, vv, _ in case.claims[0]["where"] if vv == v)
    assert restated(case, f, lut=lut)[0] != reference(case, f)[2]
