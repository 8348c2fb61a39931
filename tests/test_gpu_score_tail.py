"""The merged tail pass of k_score_coarse_sb.  A wave with two frames (k and k + 8 of an XCD slot) whose template ends in a one-chunk pass of
at most 31 live lanes scores both frames' tails in ONE pass, lanes 0..31 on the first frame and lanes 32..63 on the second.  Everything else
keeps the plain one-chunk pass: a wave with one frame, a tail of 32 lanes or more, a batch under eight frames.  Every case is compared with
the oracle (matches as a set per frame, candidates as a count) on the default kernel, the full-work build (LMX_SCORE_NO_PRUNE=1) and
k_score_coarse_u8, on the same inputs.

  640x480 (150 dwords)  a bank whose tails are 1, 4, 9, 14, 19 and 24 live lanes -- 24 is the most the geometry allows: 1200 - 1008
                        placements -- at 7 (one frame per wave), 8, 9, 16, 17 and 23 frames: slots with an even and an odd number of
                        frames, so merged and plain tails in one launch
  blank with busy       a constant frame paired with a busy one, both ways round: one half is dead from the first test
  planted instances     one whose best placement lies in the tail of the pair's second frame only (the first is blank), one in the LAST live
                        dword of the pair's first frame: its shifted nibbles come from the neighbour lane, which is not live; where the
                        best coarse placement lies is worked out on the CPU from the oracle's linear memories
  two classes           one class disabled; per-class thresholds
  704x480 (165 dwords)  tails of up to 39 lanes: the plain pass
  1280x960, two frames  every template's last pass is a two-chunk pass
The oracle's results per (set, frame, threshold) are computed once and shared."""
import numpy as np
import pytest

import class_threshold_cases as ctc
import np_restatement as R
import test_score_schedule_host as host
from linemod_pose_estimation_amd import Detector, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

THR = 84.0
MODES = {"default": ({}, "k_score_coarse_sb"), "no_prune": ({"LMX_SCORE_NO_PRUNE": "1"}, "k_score_coarse_sb"), "u8": ({"LMX_SCORE_KERNEL": "u8"}, "k_score_coarse_u8")}
CHUNK_POS, MERGE_LANES = 504, 31
WIDE = 5     # template of the 640x480 bank whose declared width is enlarged until one dword of placements is left behind the two-chunk pass
# bank arguments, frame size, scene seed of frame 0
SETS = {
    "640x480": (dict(n_templates=12, seed=92, size_range=(30.0, 80.0)), 640, 480, 1500),
    "two_classes": (dict(n_templates=8, seed=94, size_range=(30.0, 80.0), classes=["a", "b"]), 640, 480, 1600),
    "704x480": (dict(n_templates=12, seed=95, size_range=(30.0, 80.0), T=(4, 8)), 704, 480, 1700),     # 704 is no multiple of 5
    "1280x960": (dict(n_templates=8, seed=96, size_range=(30.0, 48.0)), 1280, 960, 1800),
}
BLANK, PLANT_LAST_DWORD, PLANT_TAIL = -1, -2, -3      # frame indices of the built frames
_banks, _scenes, _refs, _dets = {}, {}, {}, {}


def bank_of(name):
    if name not in _banks:
        kw = dict(SETS[name][0])
        bank = synth.make_bank(kw.pop("n_templates"), **kw)
        if name == "640x480":
            # declared extents may exceed the features' (never the other way round): 249 columns at level 1 span 32 cells of the coarsest
            # level, which leaves the template 1000 + 9 placements
            L, M = len(bank.T), len(bank.modalities)
            cid, t, f = bank.classes[0]
            t = t.copy()
            for l in range(L):
                t[(WIDE * L + l) * M:(WIDE * L + l + 1) * M, 0] = 498 >> l
            bank.classes[0] = (cid, t, f)
        _banks[name] = (bank, o.OracleDetector(bank))
    return _banks[name]


def coarse_geom(name):
    bank, _ = bank_of(name)
    _, W, H, _ = SETS[name]
    L, T = len(bank.T), bank.T[-1]
    return dict(T=T, Wc=(W >> (L - 1)) // T, Hc=(H >> (L - 1)) // T)


def positions_of(name):
    """Placements per template at the coarsest level (all classes, in bank order), from the templates' extents there."""
    bank, _ = bank_of(name)
    L, M = len(bank.T), len(bank.modalities)
    out = []
    for _, t, _ in bank.classes:
        rows = t.reshape(-1, L * M, 5)[:, (L - 1) * M:(L - 1) * M + M]
        out.append(R.template_positions(coarse_geom(name), rows[:, :, 0].max(1), rows[:, :, 1].max(1)))
    return np.concatenate(out)


def tail_lanes(positions):
    """Live lanes of the one-chunk pass behind the two-chunk passes; 0 where the last pass is a two-chunk pass."""
    rest = positions % (2 * CHUNK_POS)
    return np.where((rest >= 1) & (rest <= CHUNK_POS), -(-rest // 8), 0)


def planted(name, seed, tid, px, py):
    """A scene without instances, then template `tid` of the first class drawn with its crop origin at (px, py), as synth.make_scene draws
    its instances."""
    bank, _ = bank_of(name)
    _, W, H, _ = SETS[name]
    src = [np.ascontiguousarray(s).copy() for s in synth.make_scene(bank, W, H, seed=seed, n_instances=0)[0]]
    mt = bank.meta[bank.classes[0][0]][tid]
    assert 0 <= px and px + mt["width"] < W and 0 <= py and py + mt["height"] < H
    v = mt["verts"] + np.array([px, py], np.float64)
    m, (y0, y1, x0, x1) = synth._fill_convex((H, W), v)
    src[0][y0:y1, x0:x1][m] = (40, 55, 70)
    phi = mt["plane_label"] * (np.pi / 4)
    ys, xs = np.mgrid[y0:y1, x0:x1]
    d = float(src[1][y0:y1, x0:x1].min()) - 25.0 + 0.9 * (np.cos(phi) * (xs - v[:, 0].mean()) + np.sin(phi) * (ys - v[:, 1].mean()))
    src[1][y0:y1, x0:x1][m] = np.clip(np.rint(d), 1, 65535).astype(np.uint16)[m]
    return src


def plant_spec(which):
    """(template, px, py, first and last placement of the dwords the instance must fall in) on the 640x480 bank: the template with the
    19-lane tail, drawn in its last row of placements."""
    pos = positions_of("640x480")
    lanes = tail_lanes(pos)
    bank, _ = bank_of("640x480")
    g = coarse_geom("640x480")
    tid = int(np.flatnonzero(lanes == 19)[0])
    tail0 = (int(pos[tid]) - 1) // (2 * CHUNK_POS) * (2 * CHUNK_POS)
    lo, hi = tail0, int(pos[tid]) - 1
    if which == PLANT_LAST_DWORD:
        lo = tail0 + 8 * (int(lanes[tid]) - 1)
    row, cell = divmod((lo + hi) // 2, g["Wc"])
    return tid, 16 * cell + 2, 16 * row + 2, lo, hi


def coarse_sums(name, f, tid):
    """The coarsest-level sums of template `tid` at every placement of frame f, from the oracle's linear memories and the builder's block
    rows (the restatement of test_score_schedule_host.py) -> (sums [positions], raw threshold at THR)."""
    bank, od = bank_of(name)
    _, W, H, _ = SETS[name]
    L, M = len(bank.T), len(bank.modalities)
    t = host.rows_of(bank, W, H)
    cells = int(t["geom"]["cells"])
    od.match(scene(name, f), 90.0)
    flat = [np.concatenate([od.linear_memory(L - 1, m, (H >> (L - 1), W >> (L - 1))).astype(np.int32).reshape(8, -1),
                            np.zeros((8, cells + 8 * CHUNK_POS), np.int32)], 1) for m in range(M)]
    rows, _ = host.group_rows(t, tid, flat, cells)
    n = int(t["sinfo"][tid, 0])
    assert n == positions_of(name)[tid]
    return rows[:, :n].sum(0), host.raw_threshold(int(t["sinfo"][tid, 1]), THR)


def scene(name, f):
    if (name, f) not in _scenes:
        bank, _ = bank_of(name)
        _, W, H, seed0 = SETS[name]
        if f == BLANK:
            _scenes[name, f] = [np.full((H, W, 3), 90, np.uint8), np.full((H, W), 1200, np.uint16)]
        elif f in (PLANT_LAST_DWORD, PLANT_TAIL):
            tid, px, py, _, _ = plant_spec(f)
            _scenes[name, f] = planted(name, seed0 + 100 - f, tid, px, py)
        else:
            _scenes[name, f] = synth.make_scene(bank, W, H, seed=seed0 + f)[0]
    return _scenes[name, f]


def as_set(m):
    return sorted(zip(*(m[k].tolist() for k in ("x", "y", "similarity", "template_id", "class_index"))))


def reference(name, f, thr=THR, class_ids=()):
    """(matches as a sorted list, coarse candidates) of the oracle; never modified."""
    key = (name, f, thr, tuple(class_ids))
    if key not in _refs:
        _, od = bank_of(name)
        m = od.match(scene(name, f), thr, class_ids=class_ids)
        _refs[key] = (as_set(m), od.last_candidates())
    return _refs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_detectors():
    yield
    for det in _dets.values():
        det.close()
    _dets.clear()


def detector(name, mode, max_batch):
    """One context per (set, scoring kernel), made with the kernel's environment (read when the context is created)."""
    if (name, mode) not in _dets:
        env, kernel = MODES[mode]
        bank, _ = bank_of(name)
        _, W, H, _ = SETS[name]
        with pytest.MonkeyPatch.context() as mp:
            for k in ("LMX_SCORE_NO_PRUNE", "LMX_SCORE_KERNEL"):
                mp.delenv(k, raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            det = Detector(bank, W, H, max_batch=max_batch, max_candidates=1 << 18)
        assert det.device_kernel_name("k_score_coarse") == kernel
        _dets[name, mode] = det
    return _dets[name, mode]


def run(name, indices, mode, max_batch, class_ids=(), empty=()):
    """`indices` through enqueue / collect against the oracle; frames listed in `empty` must have no match at all, the others some."""
    n = len(indices)
    det = detector(name, mode, max_batch)
    det.upload([scene(name, f) for f in indices])
    refs = [reference(name, f, THR, class_ids) for f in indices]
    det.enqueue(n, THR, class_ids=class_ids)
    got = [as_set(g) for g in det.collect(n, cap_total=1 << 19)]
    candidates = det.stats()["candidates"]
    print(name, mode, n, "candidates", candidates, "oracle", sum(c for _, c in refs), "matches", [len(g) for g in got])
    assert candidates == sum(c for _, c in refs) > 0
    for i, f in enumerate(indices):
        if f in empty:
            assert refs[i][0] == [] and got[i] == [], i
        else:
            assert len(refs[i][0]) > 0, i          # a condition on the inputs, met on the oracle alone
            assert got[i] == refs[i][0], i
    return got


def test_the_banks_have_the_tails_the_cases_need():
    lanes = tail_lanes(positions_of("640x480"))
    assert lanes[WIDE] == 1 and set(lanes.tolist()) == {1, 4, 9, 14, 19, 24}
    assert positions_of("640x480").max() <= 1200 and 24 == -(-(1200 - 2 * CHUNK_POS) // 8)     # 24 lanes: the largest tail of 150 dwords
    assert lanes.max() <= MERGE_LANES
    lanes = tail_lanes(positions_of("two_classes"))
    assert len(lanes) == 16 and lanes.min() >= 1 and lanes.max() <= MERGE_LANES
    lanes = tail_lanes(positions_of("704x480"))
    assert coarse_geom("704x480")["Wc"] * coarse_geom("704x480")["Hc"] == 1320
    assert lanes.max() == 39 and (lanes > MERGE_LANES).sum() >= 2 and lanes.min() >= 1       # tails on both sides of the limit
    assert (tail_lanes(positions_of("1280x960")) == 0).all()


@pytest.mark.parametrize("n", (7, 8, 9, 16, 17, 23))
@pytest.mark.parametrize("mode", list(MODES))
def test_even_and_odd_slots_at_640x480(mode, n):
    run("640x480", list(range(n)), mode, 23)


@pytest.mark.parametrize("mode", list(MODES))
def test_a_blank_frame_paired_with_a_busy_one_both_ways_round(mode):
    # pairs (k, k + 8): slots 0..3 busy then blank, slots 4..7 blank then busy
    indices = [0, 1, 2, 3] + [BLANK] * 8 + [4, 5, 6, 7]
    run("640x480", indices, mode, 23, empty=(BLANK,))


@pytest.mark.parametrize("mode", list(MODES))
def test_planted_instances_in_the_tail_dwords(mode):
    g = coarse_geom("640x480")
    # slot 0: the first frame holds the instance in its tail's last live dword, the second is blank; slot 1: blank, then the instance in
    # the second frame's tail
    indices = [PLANT_LAST_DWORD, BLANK, 2, 3, 4, 5, 6, 7, BLANK, PLANT_TAIL, 10, 11, 12, 13, 14, 15]
    for f in (PLANT_LAST_DWORD, PLANT_TAIL):
        tid, px, py, lo, hi = plant_spec(f)
        # the template's best coarse placement on that frame lies in the wanted dwords and is a candidate, and the oracle finds the instance
        sums, raw_thr = coarse_sums("640x480", f, tid)
        best = int(sums.argmax())
        assert lo <= best <= hi and (sums == sums[best]).sum() == 1 and sums[best] > raw_thr, (f, best, int(sums[best]), raw_thr, lo, hi)
        assert (best // g["Wc"], best % g["Wc"]) == (py // 16, px // 16)
        assert any(m[3] == tid and m[2] >= 90.0 and abs(m[0] - px) <= 8 and abs(m[1] - py) <= 8 for m in reference("640x480", f)[0])
    got = run("640x480", indices, mode, 23, empty=(BLANK,))
    for i, f in ((0, PLANT_LAST_DWORD), (9, PLANT_TAIL)):
        tid, px, py, _, _ = plant_spec(f)
        assert any(m[3] == tid and abs(m[0] - px) <= 8 and abs(m[1] - py) <= 8 for m in got[i])


@pytest.mark.parametrize("mode", list(MODES))
def test_a_disabled_class(mode):
    run("two_classes", list(range(9)), mode, 9, class_ids=("b",))
    assert sum(reference("two_classes", f)[1] for f in range(9)) > sum(reference("two_classes", f, THR, ("b",))[1] for f in range(9))


@pytest.mark.parametrize("mode", list(MODES))
def test_per_class_thresholds(mode):
    thresholds = {"a": 88.0, "b": 80.0}
    _, od = bank_of("two_classes")
    n = 9
    key = ("two_classes", "per_class")
    if key not in _refs:
        _refs[key] = [ctc.reference(od, scene("two_classes", f), thresholds) for f in range(n)]
    refs = _refs[key]
    for c in thresholds:
        assert sum(len(r.per_class[c]) for r in refs) > 0, c
    det = detector("two_classes", mode, 9)
    det.upload([scene("two_classes", f) for f in range(n)])
    det.enqueue(n, thresholds)
    got = det.collect(n, cap_total=1 << 19)
    assert det.stats()["candidates"] == sum(r.candidates for r in refs) > 0
    for f in range(n):
        assert ctc.as_list(got[f]) == ctc.as_list(refs[f].final), f


@pytest.mark.parametrize("mode", list(MODES))
def test_tails_of_32_lanes_and_more_at_704x480(mode):
    run("704x480", list(range(9)), mode, 9)


@pytest.mark.parametrize("mode", list(MODES))
def test_two_chunk_last_pass_at_1280x960(mode):
    run("1280x960", [0, 1], mode, 2)
