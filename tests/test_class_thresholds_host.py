"""Per-class match thresholds, the parts that need no GPU: the reference the GPU tests compare against (tests/class_threshold_cases.py)
checked against the oracle's own lists, its order_key against the host merge (lmx_merge_raw), and the new entry points' argument checks
that run before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import class_threshold_cases as ctc
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd.detector import class_thresholds, merge_raw
from oracle import oracle as o


@pytest.fixture(scope="module")
def checked():
    """The bank and the three scenes the composition was worked out on."""
    bank = ctc.make_bank(32)
    od = o.OracleDetector(bank)
    return bank, od, ctc.make_frames(bank, (900, 901, 902))


def test_composition_reproduces_the_oracle_at_a_uniform_threshold(checked):
    """With every class at 80 the visit class by class is Detector::match at 80: the raw list record for record (order_key included, so the
    slots are right) and the final list in order."""
    _, od, frames = checked
    assert od.class_ids() == ctc.CLASSES
    total = 0
    for fr in frames:
        full, raw = ctc.uniform(od, fr, 80.0)
        cands = od.last_candidates()
        ref = ctc.reference(od, fr, {c: 80.0 for c in ctc.CLASSES})
        assert np.array_equal(ref.raw, raw)
        assert ctc.as_list(ref.final) == ctc.as_list(full)
        assert ref.candidates == cands
        total += len(full)
    assert total > 0


def test_mixed_thresholds_are_no_uniform_list(checked):
    """At (a: 90, b: 78, c: 84) the three frames give 9, 11 and 16 matches, every class is present, and no uniform list at 78, 84 or 90
    coincides with the mixed one (35 / 7 / 1, 29 / 6 / 1 and 90 / 14 / 2 matches)."""
    _, od, frames = checked
    refs = [ctc.reference(od, fr, ctc.THRESHOLDS) for fr in frames]
    assert [len(r.final) for r in refs] == [9, 11, 16]
    for c in ctc.CLASSES:
        assert sum(len(r.per_class[c]) for r in refs) > 0, c
    uni = [[len(ctc.uniform(od, fr, t)[0]) for t in (78.0, 84.0, 90.0)] for fr in frames]
    assert uni == [[35, 7, 1], [29, 6, 1], [90, 14, 2]]
    for r, fr in zip(refs, frames):
        for t in (78.0, 84.0, 90.0):
            assert set(ctc.as_list(r.final)) != set(ctc.as_list(ctc.uniform(od, fr, t)[0]))
        # every record obeys its own class's threshold, and the lower-threshold classes really use theirs
        for c in ctc.CLASSES:
            assert (r.per_class[c]["similarity"] >= ctc.THRESHOLDS[c]).all()
    assert any((r.per_class["b"]["similarity"] < 90.0).any() for r in refs)


def test_order_key_agrees_with_the_host_merge(checked):
    """lmx_merge_raw restores insertion order from order_key before it sorts: fed the helper's concatenated records in a shuffled order it must
    give the helper's final list, so the three-slot keys are the ones the library's host side reads.  A non-sorted visit too."""
    _, od, frames = checked
    rng = np.random.default_rng(5)
    for ids in (None, ["c", "a"]):
        ref = ctc.reference(od, frames[2], ctc.THRESHOLDS, class_ids=ids)
        assert len(ref.final) > 0
        got = merge_raw(ref.raw[rng.permutation(len(ref.raw))])
        assert ctc.as_list(got) == ctc.as_list(ref.final)


def test_entry_points_exist_and_refuse_null_arguments():
    L = _lib.lib()
    thr = (C.c_float * 3)(90.0, 78.0, 84.0)
    n = C.c_size_t()
    img = (_lib.Image * 2)()
    calls = {
        "lmx_ctx_enqueue_thresholds": lambda ctx, t: L.lmx_ctx_enqueue_thresholds(ctx, 1, t, 3, None, 0),
        "lmx_match_thresholds": lambda ctx, t: L.lmx_match_thresholds(ctx, img, 2, t, 3, None, 0, None, 0, C.byref(n)),
        "lmx_match_batch_thresholds": lambda ctx, t: L.lmx_match_batch_thresholds(ctx, 1, img, 2, t, 3, None, 0, None, 0, C.byref(n)),
        "lmx_match_masked_thresholds": lambda ctx, t: L.lmx_match_masked_thresholds(ctx, img, None, 2, t, 3, None, 0, None, 0, C.byref(n)),
        "lmx_group_submit_thresholds": lambda ctx, t: L.lmx_group_submit_thresholds(ctx, 1, t, 3, None, 0),
    }
    for name, call in calls.items():
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert call(None, thr) == _lib.LMX_ERR_INVALID_ARG, name          # null context / group
        assert b"null context" in L.lmx_last_error() or b"null group" in L.lmx_last_error(), name
        assert call(None, None) == _lib.LMX_ERR_INVALID_ARG, name         # null array
        assert b"null thresholds array" in L.lmx_last_error(), name


def test_threshold_mapping_marshalling():
    """The Python front end's mapping -> (array in class-index order, class ids to visit): absent classes are not visited, the visit follows
    class_ids when given and sorted keys otherwise, unknown keys and an empty visit are errors."""
    arr, cids, n = class_thresholds(["a", "b", "c"], {"c": 84.0, "a": 90.0})
    assert list(arr) == [90.0, 0.0, 84.0] and [cids[i] for i in range(n)] == [b"a", b"c"]
    arr, cids, n = class_thresholds(["a", "b", "c"], {"c": 84.0, "a": 90.0, "b": 78.0}, ["c", "b", "x"])
    assert list(arr) == [90.0, 78.0, 84.0] and [cids[i] for i in range(n)] == [b"c", b"b"]
    with pytest.raises(ValueError):
        class_thresholds(["a", "b"], {"z": 80.0})
    with pytest.raises(ValueError):
        class_thresholds(["a", "b"], {"a": 80.0}, ["b"])
