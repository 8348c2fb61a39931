"""Spread / linearise, coarse scoring and refinement on the device, driven with the built label images of tests/label_cases.py through
Detector.debug_enqueue_labels and compared with the oracle's match_labels: final matches per frame, the coarse candidate count, and for the
R-coarse family the coarsest level's linear memories.  What each family reaches is asserted on the CPU (tests/test_label_cases_host.py);
here every case runs as one batch (eight frames and more where the family has them: the level-by-level spread kernels, 64 stripes) and
again in calls of one and two frames (the fused spread kernel where the pair of T has one, 8 stripes, the folded read-back), on

  default    the scoring kernel the bank qualifies for (k_score_coarse_sb up to 63 coarsest-level features per template)
  no_prune   the same kernel without its bound tests (LMX_SCORE_NO_PRUNE=1)
  u8         k_score_coarse_u8 (LMX_SCORE_KERNEL=u8), likewise up to 63 features per template; banks beyond that run the generic kernel in every mode
  generic    k_score_coarse (LMX_SCORE_KERNEL=generic)
  ls_flat    the refinement reading flat spread images (LMX_LS_FLAT=1) instead of banded ones

One context per (bank, mode) and the oracle's results per frame are shared between the tests."""
import numpy as np
import pytest

import label_cases as lc
import test_label_cases_host as host
from linemod_pose_estimation_amd import Detector, _lib, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "no_prune": {"LMX_SCORE_NO_PRUNE": "1"}, "u8": {"LMX_SCORE_KERNEL": "u8"}, "generic": {"LMX_SCORE_KERNEL": "generic"},
         "ls_flat": {"LMX_LS_FLAT": "1"}}
ENV = ("LMX_SCORE_NO_PRUNE", "LMX_SCORE_KERNEL", "LMX_LS_FLAT")
SCORING = ("s_thresholds", "s_tight", "saturated", "per_class", "p", "f_depth")
REFINING = ("r_fine", "r_fine_levels3", "f_wave_split", "f_argmax", "f_equality", "f_clamps", "f_depth")
RUNS = [(f, "default") for f in lc.FAMILIES] + [(f, m) for f in SCORING for m in ("no_prune", "u8", "generic")] + [(f, "ls_flat") for f in REFINING]
FILL = 9     # frames of the batch that repeats a small case's frames
_dets = {}


@pytest.fixture(scope="module", autouse=True)
def _close_detectors():
    yield
    close_detectors()


def make_detector(case, mode, **kw):
    with pytest.MonkeyPatch.context() as mp:
        for k in ENV:
            mp.delenv(k, raising=False)
        for k, v in MODES[mode].items():
            mp.setenv(k, v)
        return Detector(case.bank, case.W, case.H, **kw)


def detector(case, mode, max_batch):
    """One context per (bank, frame size, mode) while a family runs."""
    key = (id(case.bank), case.W, case.H, mode)
    if key not in _dets:
        _dets[key] = (case.bank, make_detector(case, mode, max_batch=max_batch, max_candidates=case.max_candidates))
    return _dets[key][1]


def close_detectors():
    for _, det in _dets.values():
        det.close()
    _dets.clear()


def calls_of(case):
    """Frame indices per call: the whole case as one batch, then its frames again in calls of two and (the last, or an odd one) one frame,
    and a case of fewer than eight frames as a batch of nine."""
    n = len(case.frames)
    distinct = [f for f in range(n) if f == 0 or case.frames[f] is not case.frames[f - 1]]      # a run of one frame object is visited once
    calls = [list(range(n))] + [distinct[i:i + 2] for i in range(0, len(distinct), 2)] + [distinct[-1:]]
    if n < 8:       # a case of few frames once more as a batch of nine, its frames repeated: 64 stripes, the read-back as a launch of its own
        calls.append([distinct[i % len(distinct)] for i in range(FILL)])
    return [c for i, c in enumerate(calls) if c not in calls[:i]]


def enqueue(det, case, idx):
    labels = lc.stack(case, idx)
    if isinstance(case.threshold, dict):
        det.debug_enqueue_labels(labels, thresholds=case.threshold, class_ids=case.class_ids)
    else:
        det.debug_enqueue_labels(labels, threshold=case.threshold, class_ids=case.class_ids)


def run_case(case, mode, max_batch):
    det = detector(case, mode, max_batch)
    od = host.oracle_of(case.bank)
    L = len(case.bank.T)
    for idx in calls_of(case):
        refs = [host.reference(case, f) for f in idx]
        enqueue(det, case, idx)
        got = [host.as_set(g) for g in det.collect(len(idx), cap_total=1 << 18)]
        candidates = det.stats()["candidates"]
        assert candidates == sum(r[1] for r in refs), (case.name, mode, idx, candidates, sum(r[1] for r in refs))
        for i, f in enumerate(idx):
            assert got[i] == refs[i][0], (case.name, mode, idx, f, len(got[i]), len(refs[i][0]))
        if getattr(case, "linear_memories", False):
            thr, cids = host.visits(case)[0]
            for i, f in enumerate(idx):
                od.match_labels(case.frames[f], thr, class_ids=cids)
                for l in range(L):
                    shape = (case.H >> l, case.W >> l)
                    assert np.array_equal(det.debug_quantized(i, l, 0), case.frames[f][l][0])
                    assert np.array_equal(det.debug_linear_memory(i, l, 0), od.linear_memory(l, 0, shape)), (case.name, idx, f, l)
    return det


def qualifies(bank):
    """The unified and block tables of the u8 and sb kernels hold up to 63 coarsest-level features per template, all modalities together;
    a bank with more runs the generic kernel whatever LMX_SCORE_KERNEL says."""
    L, M = len(bank.T), len(bank.modalities)
    return all(t.reshape(-1, L * M, 5)[:, (L - 1) * M:, 4].sum(1).max() <= 63 for _, t, _ in bank.classes)


@pytest.mark.parametrize("family,mode", RUNS)
def test_family(family, mode):
    kernels = set()
    cases = lc.family(family)
    for case in cases:
        det = run_case(case, mode, max(FILL, max(len(c.frames) for c in cases if c.bank is case.bank)))
        want = {"u8": "k_score_coarse_u8", "generic": "k_score_coarse"}.get(mode, "k_score_coarse_sb") if qualifies(case.bank) else "k_score_coarse"
        assert det.device_kernel_name("k_score_coarse") == want, (case.name, mode)
        kernels.add(want)
    close_detectors()
    print(family, mode, sorted(kernels))
    if family in SCORING and mode != "generic":
        assert kernels - {"k_score_coarse"}         # the family has banks that reach the kernel the mode asks for
    if family in ("s_thresholds", "saturated"):
        assert "k_score_coarse" in kernels          # and banks of 64 .. 189 features, which only the generic kernel takes


def launches_of(det, case, idx):
    det.reset_profiling()
    enqueue(det, case, idx)
    got = det.collect(len(idx), cap_total=1 << 18)
    assert [host.as_set(g) for g in got] == [host.reference(case, f)[0] for f in idx]
    return {k: v[1] for k, v in det.kernel_times().items()}


def test_the_cases_take_the_spread_paths_they_are_named_for():
    """Launches per call, observed with profiling on (as tests/test_gpu_buffer_bytes.py does): one k_spread_linearize launch for both levels
    = the fused k_small_spread; k_pack_nibbles once per modality exactly where the coarsest level keeps byte-wide memories."""
    coarse = {c.name[len("r_coarse_"):]: c for c in lc.family("r_coarse")}
    sat = lc.family("saturated")
    p640 = next(c for c in lc.family("p") if c.W == 640 and len(c.frames) == 2)
    # (case, frames of the call, fused?, k_pack_nibbles launches)
    whole = lambda c: list(range(len(c.frames)))
    want = [(coarse["fused_nibbles"], [0], True, 0), (coarse["fused_nibbles"], [1, 2], True, 0), (coarse["fused_nibbles"], whole(coarse["fused_nibbles"]), False, 0),
            (coarse["bytes_then_pack"], [0], False, 1), (coarse["bytes_then_pack"], whole(coarse["bytes_then_pack"]), False, 1),
            (coarse["generic_odd_width"], [0, 1], False, 1), (coarse["generic_odd_width"], whole(coarse["generic_odd_width"]), False, 1),
            (sat[0], [0], True, 0), (sat[0], [0, 1], True, 0), (sat[1], [0], True, 0), (sat[1], [0, 1], True, 0),
            (sat[1], [0, 1, 0], False, 0),   # three frames: level by level
            (sat[2], [0, 1], False, 0),      # three modalities: not the one-frame chain
            (p640, [0], True, 0), (p640, [0, 1], True, 0)]
    dets = {}
    for case, idx, fused, n_pack in want:
        if id(case) not in dets:
            dets[id(case)] = make_detector(case, "default", max_batch=max(3, len(case.frames)), max_candidates=case.max_candidates)
            dets[id(case)].set_profiling(True)
        launches = launches_of(dets[id(case)], case, idx)
        assert launches["k_pack_nibbles"] == n_pack, (case.name, idx, launches)
        # a fused call spreads both levels in its one k_small_spread launch; every other call launches per level at least
        assert (launches["k_spread_linearize"] == 1) == fused and launches["k_spread_linearize"] >= 1, (case.name, idx, launches["k_spread_linearize"])
        assert launches["k_score_coarse"] == launches["k_refine"] == 1 and launches["k_color_quantize"] == launches["k_depth_quantize"] == 0, launches
    for det in dets.values():
        det.close()


@pytest.mark.parametrize("M", (1, 2, 3))
def test_saturated_frame_beyond_the_candidate_capacity(M):
    """max_candidates below the count: the overflow is reported, with the reference's count."""
    case = lc.family("saturated")[M - 1]
    want = host.reference(case, 0)[1]
    for n in (1, 2, 3):
        det = make_detector(case, "default", max_batch=3, max_candidates=want // 2)
        det.debug_enqueue_labels(lc.stack(case, [0] * n), threshold=case.threshold)
        if n * want <= 3 * (want // 2):
            got = det.collect(n, cap_total=1 << 18)
            assert [host.as_set(g) for g in got] == [host.reference(case, 0)[0]] * n
            assert det.stats()["raw_matches"] == n * want       # every candidate of the saturated frame survives
        else:
            with pytest.raises(_lib.LmxError) as e:
                det.collect(n, cap_total=1 << 18)
            assert e.value.status == _lib.LMX_ERR_OVERFLOW
        assert det.stats()["candidates"] == n * want        # counted in full, stored or not
        det.close()


def test_hook_runs_eagerly_on_a_graph_context_and_keeps_the_slot_accounting():
    case = lc.family("f_wave_split")[1]
    det = make_detector(case, "default", max_batch=len(case.frames), max_candidates=1 << 14, hipgraph=True)
    n = len(case.frames)
    refs = [host.reference(case, f) for f in range(n)]
    for _ in range(2):
        # as many enqueues in flight as the context allows, collected in order; then one too many
        for _ in range(det.max_outstanding):
            enqueue(det, case, list(range(n)))
        with pytest.raises(_lib.LmxError) as e:
            enqueue(det, case, [0])
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "outstanding" in str(e.value)
        for _ in range(det.max_outstanding):
            got = det.collect(n, cap_total=1 << 16)
            assert [host.as_set(g) for g in got] == [r[0] for r in refs]
            assert det.stats()["candidates"] == sum(r[1] for r in refs)
    enqueue(det, case, [0, 1])
    det.release()
    det.close()


def test_refusals():
    case = lc.family("f_argmax")[0]
    det = make_detector(case, "default", max_batch=2)
    L = _lib.lib()
    labels = lc.stack(case, [0, 1])
    flat = [a for lv in labels for a in lv]
    ptrs = (_lib.C.c_void_p * 4)(*[a.ctypes.data for a in flat])
    call = lambda n_frames, p, n_labels, thr=None, n_thr=0: L.lmx_ctx_debug_enqueue_labels(det.h, n_frames, p, n_labels, _lib.C.c_float(60.0), thr, n_thr, None, 0)
    INV = _lib.LMX_ERR_INVALID_ARG
    assert call(0, ptrs, 4) == INV and b"outside [1,2]" in L.lmx_last_error()
    assert call(3, ptrs, 4) == INV and b"outside [1,2]" in L.lmx_last_error()
    assert call(2, ptrs, 3) == INV and b"2 levels x 2 modalities" in L.lmx_last_error()
    assert call(2, ptrs, 5) == INV
    assert call(2, None, 4) == INV
    holed = (_lib.C.c_void_p * 4)(flat[0].ctypes.data, flat[1].ctypes.data, None, flat[3].ctypes.data)
    assert call(2, holed, 4) == INV and b"level 1, modality 0" in L.lmx_last_error()
    assert L.lmx_ctx_debug_enqueue_labels(None, 2, ptrs, 4, _lib.C.c_float(60.0), None, 0, None, 0) == INV
    thr = (_lib.C.c_float * 2)(60.0, 60.0)
    assert call(2, ptrs, 4, thr, 2) == INV and b"1 classes" in L.lmx_last_error()        # one entry per class of the bank
    nan = (_lib.C.c_float * 1)(float("nan"))
    assert call(2, ptrs, 4, nan, 1) == INV and b"not a number" in L.lmx_last_error()
    with pytest.raises(ValueError):
        det.debug_enqueue_labels([labels[0]], threshold=60.0)
    with pytest.raises(ValueError):
        det.debug_enqueue_labels(labels + [labels[1]], threshold=60.0)       # a level too many
    with pytest.raises(ValueError):
        det.debug_enqueue_labels(labels)                                     # no threshold at all
    with pytest.raises(ValueError):
        det.debug_enqueue_labels(labels, threshold=60.0, thresholds={"f": 60.0})
    with pytest.raises(ValueError):
        det.debug_enqueue_labels([labels[0], [labels[1][0][:, :-1], labels[1][1]]], threshold=60.0)
    # nothing was enqueued by a refused call, and the context still works
    det.debug_enqueue_labels(labels, threshold=60.0)
    got = det.collect(2)
    assert [host.as_set(g) for g in got] == [host.reference(case, f)[0] for f in (0, 1)]
    det.close()


@pytest.mark.parametrize("n_frames", (1, 2, 9))
def test_the_hook_runs_the_products_chain(n_frames):
    """A synth scene through upload + enqueue; its label images, read back, through the hook: the same matches, candidates and memories."""
    bank = synth.make_bank(24, seed=61, size_range=(24.0, 60.0))
    W, H = 320, 240
    frames = [synth.make_scene(bank, W, H, seed=62 + f)[0] for f in range(n_frames)]
    det = Detector(bank, W, H, max_batch=n_frames, max_candidates=1 << 15)
    det.upload(frames)
    det.enqueue(n_frames, 78.0)
    want = det.collect(n_frames)
    stats = det.stats()
    labels = [[np.stack([det.debug_quantized(f, l, m) for f in range(n_frames)]) for m in range(2)] for l in range(2)]
    memories = [det.debug_linear_memory(n_frames - 1, l, 1) for l in range(2)]
    other = Detector(bank, W, H, max_batch=n_frames, max_candidates=1 << 15)     # a context that never saw the frames
    other.debug_enqueue_labels(labels, threshold=78.0)
    got = other.collect(n_frames)
    assert sum(len(w) for w in want) > 0 and other.stats() == stats
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    for l in range(2):
        assert np.array_equal(other.debug_linear_memory(n_frames - 1, l, 1), memories[l])
    od = o.OracleDetector(bank)
    for f in range(n_frames):
        assert host.as_set(od.match_labels([[labels[l][m][f] for m in range(2)] for l in range(2)], 78.0)) == host.as_set(got[f])
    det.close()
    other.close()
