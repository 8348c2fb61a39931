"""Per-class match thresholds on the device (lmx_ctx_enqueue_thresholds and everything on top of it): a three-class bank with 11 templates per
class, so that class boundaries fall inside a four-wave scoring workgroup, matched at 90 / 78 / 84.  The yardstick is the oracle alone
(tests/class_threshold_cases.py: every class matched by itself at its own threshold, joined, std::sort, std::unique); final lists are
compared IN ORDER and the candidate count against the sum of the oracle's.  Nothing here has a tolerance, and no frame or class is skipped."""
import os
import subprocess

import numpy as np
import pytest

import class_threshold_cases as ctc
import cluster_class_cases as ccc
from conftest import ROOT
from linemod_pose_estimation_amd import Detector, NativeBank, _lib
from linemod_pose_estimation_amd.detector import cluster_matches_classes
from linemod_pose_estimation_amd.dist import DeviceGroup
from oracle import oracle as o

pytestmark = pytest.mark.gpu

# frame 0 alone already holds every class and a record of a lower-threshold class below the highest threshold; blank frames at 1 and 8
SEEDS = (902, None, 900, 903, 904, 905, 906, 907, None, 909, 910, 911, 912, 913, 914, 915, 916)
SET_A = ctc.THRESHOLDS                               # a: 90, b: 78, c: 84
SET_B = {"a": 82.0, "b": 88.0, "c": 80.0}
MODES = {"default": ({}, "k_score_coarse_sb"), "u8": ({"LMX_SCORE_KERNEL": "u8"}, "k_score_coarse_u8"), "generic": ({"LMX_SCORE_KERNEL": "generic"}, "k_score_coarse"),
         "no_prune": ({"LMX_SCORE_NO_PRUNE": "1"}, "k_score_coarse_sb")}
_state, _refs = {}, {}


def world():
    if not _state:
        bank = ctc.make_bank(11)
        _state.update(bank=bank, od=o.OracleDetector(bank), frames=ctc.make_frames(bank, SEEDS))
        assert _state["od"].class_ids() == ctc.CLASSES
    return _state["bank"], _state["od"], _state["frames"]


def ref(f, thresholds, class_ids=None, masks=None):
    """The reference of frame f; computed once, never modified."""
    key = (f, tuple(sorted(thresholds.items())), tuple(class_ids or ()), masks is not None)
    if key not in _refs:
        _, od, frames = world()
        _refs[key] = ctc.reference(od, frames[f], thresholds, class_ids=class_ids, masks=masks)
    return _refs[key]


def check_inputs(n, thresholds, class_ids=None):
    """Conditions on the inputs, met on the oracle alone before any device result is looked at: every class matched has a match in the batch
    at its own threshold; in some frame the reference differs, as a set, from the oracle's uniform list at each threshold in use; a record
    of a class below the highest threshold has a similarity below the highest threshold."""
    _, od, frames = world()
    refs = [ref(f, thresholds, class_ids) for f in range(n)]
    visit = class_ids or ctc.CLASSES
    for c in visit:
        assert sum(len(r.per_class[c]) for r in refs) > 0, c
    used = sorted({thresholds[c] for c in visit})
    assert any(all(set(ctc.as_list(r.final)) != set(ctc.as_list(ctc.uniform(od, frames[f], t)[0])) for t in used) for f, r in enumerate(refs))
    top = used[-1]
    assert any((r.per_class[c]["similarity"] < top).any() for r in refs for c in visit if thresholds[c] < top)
    return refs


def assert_lists(got, refs):
    assert len(got) == len(refs)
    for f, (g, r) in enumerate(zip(got, refs)):
        assert ctc.as_list(g) == ctc.as_list(r.final), f


def detector(n, monkeypatch=None, mode="default", **kw):
    bank, _, _ = world()
    if monkeypatch is not None:
        for k in ("LMX_SCORE_NO_PRUNE", "LMX_SCORE_KERNEL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in MODES[mode][0].items():
            monkeypatch.setenv(k, v)          # read when the context is created
    det = Detector(bank, ctc.W, ctc.H, max_batch=n, **kw)
    assert det.device_kernel_name("k_score_coarse") == MODES[mode][1]
    return det


@pytest.mark.parametrize("n", (1, 2, 5, 9, 17))
@pytest.mark.parametrize("mode", list(MODES))
def test_batches_on_every_scoring_kernel(mode, n, monkeypatch):
    """1 and 2 frames: the small chain; 5: one frame per wave; 9 and 17: the XCD grid with two frames per wave and ragged groups, blank
    frames at 1 and 8.  Through enqueue / collect and through match_batch (lmx_match_batch_thresholds)."""
    _, _, frames = world()
    refs = check_inputs(n, SET_A)
    det = detector(n, monkeypatch, mode)
    det.upload(frames[:n])
    det.enqueue(n, SET_A)
    got = det.collect(n)
    candidates = det.stats()["candidates"]
    print(mode, n, "candidates", candidates, "oracle", sum(r.candidates for r in refs), "matches", [len(g) for g in got])
    assert candidates == sum(r.candidates for r in refs) > 0
    assert_lists(got, refs)
    for f in (1, 8):
        if f < n:
            assert len(got[f]) == 0
    assert_lists(det.match_batch(frames[:n], SET_A), refs)
    if n == 1:
        assert_lists([det.match(frames[0], SET_A)], refs)
    det.close()


def test_equal_thresholds_are_the_uniform_call():
    """All thresholds equal to t: records, order and lmx_ctx_stats of enqueue(t) on the same upload."""
    _, _, frames = world()
    n = 9
    det = detector(n)
    det.upload(frames[:n])
    for t in (84.0, 78.0):
        det.enqueue(n, t)
        a, sa = det.collect(n), det.stats()
        det.enqueue(n, {c: t for c in ctc.CLASSES})
        b, sb = det.collect(n), det.stats()
        assert sa == sb and sa["candidates"] > 0 and sum(len(m) for m in a) > 0
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    det.close()


def test_class_ids_in_another_order_and_a_class_left_out():
    _, _, frames = world()
    n = 5
    ids = ["c", "a"]
    refs = check_inputs(n, SET_B, ids)
    det = detector(n)
    det.upload(frames[:n])
    det.enqueue(n, SET_B, class_ids=ids)
    got = det.collect(n)
    assert det.stats()["candidates"] == sum(r.candidates for r in refs)
    assert_lists(got, refs)
    assert all((g["class_index"] != 1).all() for g in got)
    # a mapping that lacks a class leaves it out too, and visits the rest in sorted order
    sub = {"a": SET_B["a"], "c": SET_B["c"]}
    refs = [ref(f, sub, ["a", "c"]) for f in range(n)]
    det.enqueue(n, sub)
    assert_lists(det.collect(n), refs)
    det.close()


def test_a_threshold_above_100_silences_its_class_only():
    _, _, frames = world()
    n = 5
    thr = dict(SET_A, b=100.5)
    base = check_inputs(n, SET_A)
    refs = [ref(f, thr) for f in range(n)]
    assert all(len(r.per_class["b"]) == 0 for r in refs)
    det = detector(n)
    det.upload(frames[:n])
    det.enqueue(n, thr)
    got = det.collect(n)
    assert_lists(got, refs)
    for g, r0 in zip(got, base):
        rest = r0.final[r0.final["class_index"] != 1]
        assert sorted(ctc.as_list(g)) == sorted(ctc.as_list(rest))
    det.close()


@pytest.mark.parametrize("hipgraph", (False, True))
def test_outstanding_enqueues_with_different_thresholds(hipgraph):
    """Two enqueues in flight with different threshold sets, collected afterwards; then four more steps, pipelined, in which every output
    slot sees both sets in turn -- with hipgraph=True the second use of a slot replays its captured chain, which must read the new values."""
    _, _, frames = world()
    n = 5
    ra, rb = check_inputs(n, SET_A), check_inputs(n, SET_B)
    det = detector(n, hipgraph=hipgraph)
    assert det.max_outstanding == 2
    det.upload(frames[:n])
    det.enqueue(n, SET_A)
    det.enqueue(n, SET_B)
    assert_lists(det.collect(n), ra)
    assert det.stats()["candidates"] == sum(r.candidates for r in ra)
    assert_lists(det.collect(n), rb)
    assert det.stats()["candidates"] == sum(r.candidates for r in rb)
    steps = [(SET_B, rb), (SET_A, ra), (SET_A, ra), (SET_B, rb)]     # slot 0: A, B, A; slot 1: B, A, B
    det.enqueue(n, steps[0][0])
    for k in range(1, len(steps) + 1):
        if k < len(steps):
            det.enqueue(n, steps[k][0])
        assert_lists(det.collect(n), steps[k - 1][1])
    # a uniform enqueue between two per-class ones keeps its own chain
    det.enqueue(n, 84.0)
    det.enqueue(n, SET_A)
    _, od, _ = world()
    uni = det.collect(n)
    for f in range(n):
        assert ctc.as_list(uni[f]) == ctc.as_list(ctc.uniform(od, frames[f], 84.0)[0])
    assert_lists(det.collect(n), ra)
    det.close()


def test_bad_arguments_enqueue_nothing():
    _, _, frames = world()
    L = _lib.lib()
    det = detector(1)
    det.upload(frames[:1])
    import ctypes as C
    good = (C.c_float * 3)(90.0, 78.0, 84.0)
    nan = (C.c_float * 3)(90.0, float("nan"), 84.0)
    for args, word in (((None, 3), "null"), ((good, 2), "3 classes"), ((good, 4), "3 classes"), ((nan, 3), "not a number")):
        assert L.lmx_ctx_enqueue_thresholds(det.h, 1, args[0], args[1], None, 0) == _lib.LMX_ERR_INVALID_ARG
        assert word in L.lmx_last_error().decode(), word
    with pytest.raises(_lib.LmxError, match="nothing|outstanding|enqueue"):
        det.collect(1)                              # nothing was enqueued
    det.enqueue(1, SET_A)
    assert_lists(det.collect(1), [ref(0, SET_A)])
    det.close()


def test_match_masked_with_thresholds():
    _, od, frames = world()
    masks = [np.zeros((ctc.H, ctc.W), np.uint8), None]
    masks[0][:, : ctc.W * 2 // 3] = 255
    r = ctc.reference(od, frames[0], SET_A, masks=masks)
    full = ref(0, SET_A)
    assert 0 < len(r.final) and ctc.as_list(r.final) != ctc.as_list(full.final)
    det = detector(1)
    got = det.match_masked(frames[0], masks, SET_A)
    assert ctc.as_list(got) == ctc.as_list(r.final)
    assert det.stats()["candidates"] == r.candidates
    det.close()


@pytest.mark.parametrize("frame_groups", (1, 2))
def test_device_group_equals_the_single_context(frame_groups):
    """Two members on one device as 1 x 2 (two template shards) and as 2 x 1 (two frame groups): every member forwards the same array."""
    bank, _, frames = world()
    n = 5
    refs = check_inputs(n, SET_A)
    det = detector(n)
    det.upload(frames[:n])
    det.enqueue(n, SET_A)
    single = det.collect(n)
    det.close()
    assert_lists(single, refs)
    g = DeviceGroup(bank, ctc.W, ctc.H, n_members=2, devices=[0, 0], max_batch=n, collective="peer_copy", frame_groups=frame_groups)
    assert g.size == 2 and g.frame_groups == frame_groups
    g.upload(frames[:n])
    g.submit(n, SET_A)
    g.submit(n, SET_B)
    got_a, got_b = g.finish(n), g.finish(n)
    g.close()
    for x, y in zip(got_a, single):
        assert np.array_equal(x, y)
    assert_lists(got_b, [ref(f, SET_B) for f in range(n)])


def sidecars(bank, names):
    by_name = {cid: t for cid, t, _ in bank.classes}
    rows = len(bank.T) * len(bank.modalities)
    out = []
    for c, cid in enumerate(names):
        t = by_name[cid][::rows]
        rects = np.stack([np.zeros(len(t)), np.zeros(len(t)), t[:, 0], t[:, 1]], 1).astype(np.int32)
        dists = 0.55 + 0.1 * ((np.arange(len(t)) + c) % 3) + 0.013 * c
        out.append(ccc.Side(dists, rects, 32, 0.5, 0.1, 0))       # size threshold 0: frame 0 gives clusters of all three classes, one of two members
    return out


def test_cluster_chain_behind_a_thresholds_enqueue():
    """set_cluster_sidecar_class + collect_clusters_classes behind a thresholds enqueue: the matches are the reference's, clusters and members
    what cluster_matches_classes makes of that list."""
    bank, _, frames = world()
    n = 2
    refs = check_inputs(n, SET_A)
    det = detector(n)
    sides = sidecars(bank, det.classIds())
    for c, s in enumerate(sides):
        det.set_cluster_sidecar_class(c, s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh)
    det.upload(frames[:n])
    det.enqueue(n, SET_A)
    out = det.collect_clusters_classes(n)
    assert_lists([fr[0] for fr in out], refs)
    m, _, _, cl, k, mem = out[0]
    want_c, want_k, want_mem = cluster_matches_classes(m, [(s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh) for s in sides])
    assert len(cl) > 0 and len(set(k.tolist())) > 1
    assert np.array_equal(cl, want_c) and np.array_equal(k, want_k)
    n_mem = int(cl["member_count"].sum())
    assert np.array_equal(mem[:n_mem], want_mem[:n_mem])
    det.close()


def test_cpp_caller_prints_what_python_computes(tmp_path):
    """tests/cpp/class_thresholds_main.cpp: lmx::linemod::Detector::match with a std::map of two classes at two thresholds."""
    bank, _, frames = world()
    thr = {"b": SET_A["b"], "a": SET_A["a"]}
    r = ref(0, thr, ["a", "b"])
    assert len(r.per_class["a"]) > 0 and len(r.per_class["b"]) > 0
    bank_yml = str(tmp_path / "bank.yml")
    NativeBank.from_bank(bank).save_yaml(bank_yml)
    for k, fr in enumerate(frames[0]):
        np.ascontiguousarray(fr).tofile(str(tmp_path / ("source_%d.bin" % k)))
    exe = str(tmp_path / "class_thresholds_main")
    csrc = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "class_thresholds_main.cpp"), "-o", exe, "-L", csrc, "-llmx", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([exe, bank_yml, str(tmp_path), str(ctc.W), str(ctc.H), "b", "%g" % thr["b"], "a", "%g" % thr["a"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    det = detector(1)
    got = det.match(frames[0], thr)
    det.close()
    assert ctc.as_list(got) == ctc.as_list(r.final)
    names = det.classIds()
    lines = ["matches %d" % len(got)] + ["%d %d %.9g %s %d" % (m["x"], m["y"], m["similarity"], names[m["class_index"]], m["template_id"]) for m in got]
    assert res.stdout.strip().split("\n") == lines
