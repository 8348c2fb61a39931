"""Pose refinement under a schedule, without a device: the shared header's refine_job_staged and check_schedule (csrc/lmx_pose_refine.hpp,
built with plain g++ from tests/cpp/pose_refine_staged_host.cpp) against the numpy restatement of tests/pose_refine_staged_cases.py -- the
integer sums of every pass and every byte of the record; the statuses a schedule adds; the identities with the unstaged definition; the
ground-truth case; the same C++ file's main() under AddressSanitizer + UBSan as a child process; the setter's refusals, which need no
device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pose_refine_cases as prc
import pose_refine_staged_cases as psc
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd import POSE_REFINE_DTYPE, DepthTemplates


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return psc.build_host(tmp_path_factory.mktemp("prshost"))


def _both(host, P, stages, crop, rect_xy, scene, x, y, what):
    """The restatement and the header on one job, equal in every sum row and every byte -> (record dict, sums, trace)."""
    rec, sums, trace = psc.np_refine_staged(P, stages, crop, rect_xy, scene, x, y)
    got, got_sums = psc.host_refine_staged(host, P, stages, crop, rect_xy, scene, x, y, POSE_REFINE_DTYPE)
    assert np.array_equal(sums, got_sums), (what, np.nonzero((sums != got_sums).any(1))[0][:3])
    want = prc.record_array(rec, POSE_REFINE_DTYPE)
    for k in POSE_REFINE_DTYPE.names:
        assert want[k].tobytes() == got[k].tobytes(), (what, k, want[k], got[k])
    assert want.tobytes() == got.tobytes(), what
    return rec, sums, trace


def test_header_equals_the_numpy_restatement_and_the_statuses(host):
    scenes = psc.scenes()
    by_name = {}
    for j in psc.constructed_jobs():
        rec, sums, trace = _both(host, j.P, j.stages, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, j.name)
        for k, v in (j.expect or {}).items():
            assert rec[k] == v, (j.name, k, rec[k], v)
        assert rec["n_model"] == int((j.crop != 0).sum())
        assert not sums[len(trace):].any() and len(trace) == rec["iterations"] + 1          # one pass per iteration and the one that ended it
        assert sums[len(trace) - 1, 0] == rec["n_pairs_last"] and trace[-1][0] == rec["reserved"]
        by_name[j.name] = (rec, sums, trace)
    recs = {n: v[0] for n, v in by_name.items()}
    # what the set of cases covers
    rec, sums, trace = by_name["converged_in_stage_0"]
    n0 = sum(1 for s, _ in trace if s == 0)
    assert 1 <= n0 < 64 and trace[n0][0] == 1 and rec["iterations"] > n0                    # CONVERGED in a stage that is not the last, and on it went
    assert any(r["status"] == prc.LOST and r["reserved"] == 0 for r in recs.values())
    rec, sums, trace = by_name["lost_in_stage_1"]
    assert [s for s, _ in trace] == [0, 0, 0, 0, 1] and sums[4, 0] < 27 <= sums[3, 0]      # LOST in pass 0 of stage 1, with the pose stage 0 left
    assert rec["R"] != [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    rec, sums, trace = by_name["four_stages"]
    assert sorted(set(s for s, _ in trace)) == [0, 1, 2, 3] and rec["reserved"] == 3
    assert [n for _, n in trace] == sorted((n for _, n in trace))                            # every stage selects more pixels than the one before
    # one selected pixel: pass 0 of stage 0 pairs at most that one
    for name in ("crop_3x3_stride_8", "crop_8x8_stride_8", "crop_3x3_stride_4"):
        assert by_name[name][2] == [(0, 1)] and by_name[name][1][0, 0] <= 1 and recs[name]["R"] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    # the wide crop: most of it hangs off the scene, and the lattice still reaches the part that does not
    rec, sums, trace = by_name["crop_530x3_stride_2"]
    assert trace[0][1] < rec["n_model"] // 3 and 3 <= sums[0, 0] < 200 and rec["iterations"] >= 2
    # the coarse stage's window matters over holes
    assert not np.array_equal(by_name["coarse_radius_0"][1][0], by_name["coarse_radius_2"][1][0])
    assert not np.array_equal(by_name["wide_coarse_radius_0"][1][0], by_name["wide_coarse_radius_2"][1][0])


def test_identities_with_the_unstaged_definition(host):
    scenes = prc.scenes()
    # one stage of stride 1 that repeats the parameters: refine_job and np_refine in every byte, on every case of the unstaged suite
    for j in prc.constructed_jobs():
        want, want_sums = psc.host_refine_plain(host, j.P, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE)
        for got, got_sums in (psc.host_refine_staged(host, j.P, [psc.stage_of_params(j.P)], j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE),
                              psc.host_refine_plain(host, j.P, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE, as_single_stage=True)):
            assert got.tobytes() == want.tobytes() and np.array_equal(got_sums, want_sums), j.name
        assert want["reserved"][0] == 0
    j = [j for j in prc.constructed_jobs() if j.name == "holes"][0]
    rec, sums = prc.np_refine(j.P, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y)
    got, got_sums = psc.host_refine_staged(host, j.P, [psc.stage_of_params(j.P)], j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE)
    assert prc.record_array(rec, POSE_REFINE_DTYPE).tobytes() == got.tobytes() and np.array_equal(sums, got_sums)
    # A x 10 then A x 10 with eps 0 is A x 20 in every field but `reserved`, and runs 21 passes
    g = prc.ground_truth_case()
    bx, by = g["rect_b"][:2]
    P = prc.make_params(prc.GT_CAM, prc.GT_CAM, eps_rot_rad=0.0, eps_trans_mm=0.0, max_iterations=20)
    A = psc.make_stage(eps_rot_rad=0.0, eps_trans_mm=0.0, max_iterations=10)
    two, two_sums = psc.host_refine_staged(host, P, [A, A], g["crop"], g["rect"][:2], g["scene"], bx, by, POSE_REFINE_DTYPE)
    one, one_sums = psc.host_refine_plain(host, P, g["crop"], g["rect"][:2], g["scene"], bx, by, POSE_REFINE_DTYPE)
    assert np.array_equal(two_sums, one_sums) and two_sums[20].any() and two_sums.shape == (21, 17)
    assert two["reserved"][0] == 1 and one["reserved"][0] == 0 and two["iterations"][0] == 20
    for k in POSE_REFINE_DTYPE.names:
        if k != "reserved":
            assert two[k].tobytes() == one[k].tobytes(), k


def test_check_schedule_refuses_each_rule_and_admits_the_extremes(host):
    good = psc.make_stage()
    ok = lambda stages: psc.check_schedule(host, stages)
    assert ok([good]) and ok([good] * 4)
    assert not ok([]) and not ok([good] * 5)
    nan = float("nan")
    for bad in (dict(max_dist_mm=0.0), dict(max_dist_mm=1024.5), dict(max_dist_mm=nan), dict(eps_rot_rad=-1e-9), dict(eps_rot_rad=nan), dict(eps_trans_mm=-1.0),
                dict(eps_trans_mm=nan), dict(max_iterations=-1), dict(max_iterations=65), dict(search_radius=-1), dict(search_radius=3), dict(stride=0), dict(stride=3),
                dict(stride=16), dict(stride=-2)):
        assert not ok([dict(good, **bad)]), bad
        assert not ok([good, dict(good, **bad)]) and not ok([dict(good, **bad), good]), bad
    # a stage in front of the last needs an iteration; the last does not
    zero = dict(good, max_iterations=0)
    assert ok([zero]) and ok([good, zero]) and not ok([zero, good]) and not ok([good, zero, good])
    for g in (1, 2, 4, 8):
        assert ok([dict(good, stride=g, max_dist_mm=1024.0, max_iterations=64, search_radius=2, eps_rot_rad=0.0, eps_trans_mm=0.0)] * 4), g
    assert ok([dict(good, max_iterations=1, search_radius=0), good])


def test_ground_truth_under_the_schedule(host):
    """Conditions, not measurements; the figures are recorded in profiles/pose_refine_staged.txt."""
    g = prc.ground_truth_case()
    bx, by = g["rect_b"][:2]
    stages = psc.parse_schedule(psc.GT_SCHEDULES[0])
    npx = int((g["crop"] != 0).sum())
    for (x, y) in ((bx, by), (bx + 1, by), (bx, by + 1)):
        P = prc.make_params(prc.GT_CAM, prc.GT_CAM)
        rec, _, trace = _both(host, P, stages, g["crop"], g["rect"][:2], g["scene"], x, y, ("ground truth", x, y))
        err = prc.pose_errors(*prc.compose(g["R_a"], g["distance"], rec), g["R_b"], g["T_b_m"])
        others = {}
        for it in (0, 20):
            plain, _ = psc.host_refine_plain(host, prc.make_params(prc.GT_CAM, prc.GT_CAM, max_iterations=it), g["crop"], g["rect"][:2], g["scene"], x, y, POSE_REFINE_DTYPE)
            others[it] = prc.pose_errors(*prc.compose(g["R_a"], g["distance"], plain[0]), g["R_b"], g["T_b_m"])
        print("match (%d, %d), %s: status %d in stage %d after %d iterations, %.2f full passes of pixel work, rms %.4f -> %.4f mm, rotation error %.4f deg, "
              "translation error %.4f mm; single stage of 20: %.4f deg %.4f mm; placement: %.4f deg %.4f mm"
              % (x, y, psc.GT_SCHEDULES[0], rec["status"], rec["reserved"], rec["iterations"], sum(n for _, n in trace) / npx, rec["rms_first_mm"], rec["rms_last_mm"],
                 err[0], err[1], others[20][0], others[20][1], others[0][0], others[0][1]))
        assert rec["status"] in (prc.CONVERGED, prc.MAX_ITERATIONS) and rec["reserved"] == 1
        assert rec["rms_last_mm"] < rec["rms_first_mm"]
        assert err[0] < others[0][0] and err[1] < others[0][1], (err, others)


def test_border_cases_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "pose_refine_staged_host")
    subprocess.check_call(["g++"] + psc.HOST_FLAGS + san + [psc.HOST_SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "pose_refine_staged_host ok" in res.stdout


def test_the_setter_without_a_device(host):
    """The schedule lives on the host: setting, reading and refusing it touch no device."""
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    assert C.sizeof(_lib.PoseRefineStage) == host.prs_host_stage_bytes() == 40
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16)])
    assert t.refine_schedule == []
    two = psc.parse_schedule("4:20:10:1,1:3:10:1")
    t.set_refine_schedule(two)
    assert t.refine_schedule == two
    nan = float("nan")
    for bad in ([dict(two[0], stride=3), two[1]], [two[0], dict(two[1], max_dist_mm=nan)], [dict(two[0], max_iterations=0), two[1]], two * 3,
                [dict(two[0], search_radius=3)], [dict(two[0], eps_rot_rad=-1.0)], [dict(two[0], eps_trans_mm=nan)], [dict(two[0], max_iterations=65)]):
        with pytest.raises(_lib.LmxError) as e:
            t.set_refine_schedule(bad)
        assert e.value.status == INV
        assert t.refine_schedule == two, bad                                                 # the previous schedule stays
    arr = (_lib.PoseRefineStage * 4)(*[_lib.PoseRefineStage(10.0, 1e-5, 1e-3, 5, 1, 1, 0)] * 4)
    n = C.c_int32(0)
    assert L.lmx_depth_templates_set_refine_schedule(None, arr, 1) == INV and b"null" in L.lmx_last_error()
    assert L.lmx_depth_templates_set_refine_schedule(t.h, None, 1) == INV and b"stages is null" in L.lmx_last_error()
    assert L.lmx_depth_templates_set_refine_schedule(t.h, arr, 5) == INV and L.lmx_depth_templates_set_refine_schedule(t.h, arr, -1) == INV
    arr[1].reserved = 7
    assert L.lmx_depth_templates_set_refine_schedule(t.h, arr, 2) == INV and b"reserved" in L.lmx_last_error()
    assert L.lmx_depth_templates_set_refine_schedule(t.h, arr, 1) == _lib.LMX_OK              # the stage with the bad field is not part of it
    assert L.lmx_depth_templates_get_refine_schedule(t.h, None, C.byref(n)) == INV and L.lmx_depth_templates_get_refine_schedule(None, arr, C.byref(n)) == INV
    assert L.lmx_depth_templates_get_refine_schedule(t.h, arr, None) == INV
    assert len(t.refine_schedule) == 1 and t.refine_schedule[0]["max_iterations"] == 5
    with pytest.raises(ValueError):
        t.set_refine_schedule([dict(stride=2)])
    # append keeps the destination's schedule, whatever the source holds
    other = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16)])
    other.set_refine_schedule(two)
    t.append(other)
    assert len(t) == 2 and len(t.refine_schedule) == 1
    t.set_refine_schedule(None)
    assert t.refine_schedule == []
    t.set_refine_schedule(two)
    t.set_refine_schedule([])
    assert t.refine_schedule == []
    t.close()
