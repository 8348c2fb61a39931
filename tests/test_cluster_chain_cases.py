"""The constructed cases of tests/cluster_cases.py through the HOST path (no GPU): lmx_merge_raw per frame, then lmx_cluster_matches,
against the cases' library-independent reference (numpy + the real std::sort + the oracle's restatement of the reference's
rcd_voting / cluster_filter / cluster_scoring / nonMaximaSuppressionUsingIOU, /root/reference/src/rgbdDetector.cpp:36-144, 462-574).
This validates the cases where no device is needed and carries the host coverage to the same edges the device test
(tests/test_gpu_cluster_chain.py) pins: the origin, score ties beyond 16 clusters, IoU == 0.4f, ring boundaries, the size filter."""
import numpy as np
import pytest

import cluster_cases as cc
from linemod_pose_estimation_amd import _lib, merge_raw
from linemod_pose_estimation_amd.detector import cluster_matches


def check_matches(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k in cc.FIELDS:
        assert np.array_equal(got[k], ref[k]), (what, k)


def check_clusters(got_c, got_mem, ref, what):
    assert len(got_c) == len(ref.clusters), (what, len(got_c), len(ref.clusters))
    for k in cc.CLUSTER_FIELDS:
        assert np.array_equal(got_c[k], ref.clusters[k]), (what, k)
    assert np.array_equal(got_mem[:len(ref.members)], ref.members), (what, "members")


def host_frame(case, f, ref):
    """One frame through merge_raw + cluster_matches, compared in full.  The host takes frames of any size and rings of any range;
    a template id outside the side-car is LMX_ERR_INVALID_ARG."""
    what = (case.name, f)
    m = merge_raw(case.records[case.records["frame"] == f])
    check_matches(m, ref.matches, what)
    if ref.clusters is None:
        with pytest.raises(_lib.LmxError) as e:
            cluster_matches(m, case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG, what
        return
    c, mem = cluster_matches(m, case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)
    check_clusters(c, mem, ref, what)


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_constructed_case_on_the_host_path(name):
    case = cc.case_by_name(name)
    ref = cc.reference(case)
    for f in range(case.n_frames):
        host_frame(case, f, ref[f])


def test_arrival_order_does_not_matter_on_the_host_path():
    case = cc.case_by_name("arrival_order")
    ref = cc.reference(case)
    for seed in (1, 2, 3):
        sh = cc.shuffled(case, seed)
        assert not np.array_equal(sh.records["order_key"], case.records["order_key"])
        for f in range(case.n_frames):
            host_frame(sh, f, ref[f])


def test_random_draws_on_the_host_path():
    sizes = []
    for seed in cc.RANDOM_SEEDS:
        case = cc.random_case(seed)
        ref = cc.reference(case)
        for f in range(case.n_frames):
            assert ref[f].status == 0                      # within 2048 records, inside the side-car: the device takes all of them too
            host_frame(case, f, ref[f])
            sizes.append((ref[f].n_records, len(ref[f].clusters)))
    sizes = np.asarray(sizes)
    # the draws reach empty and full frames, and frames with one cluster and with many
    assert (sizes[:, 0] == 0).any() and (sizes[:, 0] > 1500).any() and (sizes[:, 1] == 0).any() and (sizes[:, 1] > 16).any()


def test_device_hook_validates_before_it_touches_a_device():
    """lmx_debug_device_finalize_cluster refuses what the kernel's LDS layout cannot hold (x, y beyond int16, class_index beyond uint16),
    n_frames outside 1..8 and the parameters lmx_ctx_set_cluster_sidecar refuses -- all before a device is looked for."""
    from conftest import has_gpu
    from linemod_pose_estimation_amd.detector import debug_device_finalize_cluster as hook
    case = cc.case_by_name("iou_boundary")
    args = (case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)

    def refused(records, n_frames, *a):
        with pytest.raises(_lib.LmxError) as e:
            hook(records, n_frames, *a)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG, str(e.value)

    for n_frames in (0, -1, 9):
        refused(case.records, n_frames, *args)
    for field, value in (("x", 32768), ("x", -32769), ("y", 32768), ("y", -32769), ("class_index", 65536), ("class_index", -1)):
        bad = case.records.copy()
        bad[field][1] = value
        refused(bad, case.n_frames, *args)
    refused(case.records, case.n_frames, case.dists, case.rects, 0, case.rmin, case.rstep, case.thresh)        # step
    refused(case.records, case.n_frames, case.dists, case.rects, case.step, case.rmin, case.rstep, -1)        # threshold
    refused(case.records, case.n_frames, case.dists, case.rects, case.step, case.rmin, 0.0, case.thresh)      # ring step
    refused(case.records, case.n_frames, [np.inf], case.rects, case.step, case.rmin, case.rstep, case.thresh)  # no usable ring
    if not has_gpu():
        with pytest.raises(_lib.LmxError) as e:
            hook(case.records, case.n_frames, *args)
        assert e.value.status == _lib.LMX_ERR_NO_DEVICE
