"""Point-to-plane pose refinement without a device: the shared header's refine_job_plane, solve_plane and check_plane
(csrc/lmx_pose_refine.hpp, built with plain g++ from tests/cpp/pose_refine_plane_host.cpp) against the numpy restatement of
tests/pose_refine_plane_cases.py -- both sum arrays of every pass as integers and every byte of the record; the ways a step can go, each
asserted to occur; the identities with the point-to-point definition; the ground-truth conditions; the same C++ file's main() under
AddressSanitizer + UBSan as a child process; the setter's refusals, which need no device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pose_refine_cases as prc
import pose_refine_plane_cases as ppc
import pose_refine_staged_cases as psc
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd import POSE_REFINE_DTYPE, DepthTemplates


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ppc.build_host(tmp_path_factory.mktemp("prphost"))


def _both(host, P, stages, shifts, crop, rect_xy, scene, normals, x, y, what):
    """The restatement and the header on one job, equal in every sum row and every byte -> (record dict, sums, plane sums, trace)."""
    rec, sums, plane, trace = ppc.np_refine_plane(P, stages, shifts, crop, rect_xy, scene, normals, x, y)
    got, got_sums, got_plane = ppc.host_refine_plane(host, P, stages, shifts, crop, rect_xy, scene, normals, x, y, POSE_REFINE_DTYPE)
    assert np.array_equal(sums, got_sums), (what, np.nonzero((sums != got_sums).any(1))[0][:3])
    assert np.array_equal(plane, got_plane), (what, np.nonzero((plane != got_plane).any(1))[0][:3])
    want = prc.record_array(rec, POSE_REFINE_DTYPE)
    for k in POSE_REFINE_DTYPE.names:
        assert want[k].tobytes() == got[k].tobytes(), (what, k, want[k], got[k])
    assert want.tobytes() == got.tobytes(), what
    return rec, sums, plane, trace


def test_header_equals_the_numpy_restatement_and_every_route_occurs(host):
    scenes, normals = ppc.scenes(), ppc.scene_normal_maps()
    by_name = {}
    for j in ppc.constructed_jobs():
        rec, sums, plane, trace = _both(host, j.P, j.stages, j.shifts, j.crop, j.rect_xy, scenes[j.scene], normals[j.normals], j.x, j.y, j.name)
        assert len(trace) == rec["iterations"] + 1 and not sums[len(trace):].any() and not plane[len(trace):].any(), j.name
        assert (plane[:, 0] <= sums[:, 0]).all(), j.name
        shifts = list(j.shifts) + [-1] * 4
        for row, (si, _, route) in enumerate(trace):
            assert (route == ppc.POINT or route is None) if shifts[si] < 0 else route != ppc.POINT, (j.name, row)
            if shifts[si] < 0:
                assert not plane[row].any(), (j.name, row)                                        # a -1 stage leaves its plane rows alone
        by_name[j.name] = (rec, sums, plane, trace)
    routes = lambda name: [r for _, _, r in by_name[name][3]]
    # some pass pairs more pixels than hold a valid normal, and some normal
    assert any(((p[:, 0] > 0) & (p[:, 0] < s[:, 0])).any() for _, s, p, _ in by_name.values())
    # each way a step can go
    assert ppc.FEW in routes("few_normals") and 0 < by_name["few_normals"][2][0, 0] < 300 <= by_name["few_normals"][1][0, 0]
    assert set(routes("all_invalid")) == {ppc.FEW, None}
    assert ppc.FALLBACK in routes("singular_row") and by_name["singular_row"][2][0, 0] >= 3
    for name in ("crop_33x37_shift_0", "crop_33x37_shift_4", "crop_33x37_shift_8", "crop_33x37_shift_20", "flat_shift_20", "holes", "sparse"):
        assert ppc.PLANE in routes(name), name
    assert [r for r in routes("flat_shift_20") if r] == [ppc.PLANE] * by_name["flat_shift_20"][0]["iterations"]   # the point term alone keeps it definite
    # the shift matters: other bytes for other weights
    recs = [prc.record_array(by_name["crop_33x37_shift_%d" % k][0], POSE_REFINE_DTYPE).tobytes() for k in (0, 4, 8, 20)]
    assert len(set(recs)) == 4
    # the stage mixes ran every stage, the metric following the stage
    for name, want in (("coarse_plane_fine_point", [0, 1]), ("point_then_plane", [0, 1]), ("four_alternating", [0, 1, 2, 3])):
        rec, sums, plane, trace = by_name[name]
        assert sorted(set(s for s, _, _ in trace)) == want and rec["reserved"] == want[-1], name
        assert any(r == ppc.PLANE for _, _, r in trace) and any(r == ppc.POINT for _, _, r in trace), name


def test_identities_with_the_point_to_point_definition(host):
    scenes, normals = ppc.scenes(), ppc.scene_normal_maps()
    by = {j.name: j for j in ppc.constructed_jobs()}
    # a normal map without a valid pixel: the point-to-point record, byte for byte, and its 17 sums
    j = by["all_invalid"]
    got, got_sums, got_plane = ppc.host_refine_plane(host, j.P, None, j.shifts, j.crop, j.rect_xy, scenes[j.scene], normals[j.normals], j.x, j.y, POSE_REFINE_DTYPE)
    want, want_sums = ppc.host_refine_point(host, j.P, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE)
    assert got.tobytes() == want.tobytes() and np.array_equal(got_sums, want_sums) and not got_plane.any()
    assert want["iterations"][0] == j.P["max_iterations"]
    # every shift -1 (with or without a normal map): refine_job / refine_job_staged in every byte, on the cases of both earlier suites
    for job in prc.constructed_jobs():
        want, want_sums = ppc.host_refine_point(host, job.P, job.crop, job.rect_xy, scenes[job.scene], job.x, job.y, POSE_REFINE_DTYPE)
        for nrm in (None, normals[job.scene]):
            got, got_sums, got_plane = ppc.host_refine_plane(host, job.P, None, [-1], job.crop, job.rect_xy, scenes[job.scene], nrm, job.x, job.y, POSE_REFINE_DTYPE)
            assert got.tobytes() == want.tobytes() and np.array_equal(got_sums, want_sums) and not got_plane.any(), job.name
    for job in psc.constructed_jobs():
        rec, sums, _ = psc.np_refine_staged(job.P, job.stages, job.crop, job.rect_xy, scenes[job.scene], job.x, job.y)
        got, got_sums, got_plane = ppc.host_refine_plane(host, job.P, job.stages, [], job.crop, job.rect_xy, scenes[job.scene], None, job.x, job.y, POSE_REFINE_DTYPE)
        assert got.tobytes() == prc.record_array(rec, POSE_REFINE_DTYPE).tobytes() and np.array_equal(got_sums, sums) and not got_plane.any(), job.name
    # the 17 sums of a plane pass are those of the point pass under the same pose: pass 0 of any job
    j = by["holes"]
    _, s_plane, _ = ppc.host_refine_plane(host, j.P, None, [8], j.crop, j.rect_xy, scenes[j.scene], normals[j.normals], j.x, j.y, POSE_REFINE_DTYPE)
    _, s_point = ppc.host_refine_point(host, j.P, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE)
    assert np.array_equal(s_plane[0], s_point[0]) and not np.array_equal(s_plane[1], s_point[1])


def test_check_plane_refuses_each_rule(host):
    ok = lambda shifts: ppc.check_plane(host, shifts)
    assert ok([]) and ok([-1]) and ok([0]) and ok([20]) and ok([8, -1, 0, 20]) and ok([-1] * 4)
    assert not ok([21]) and not ok([-2]) and not ok([8, 21]) and not ok([0, 0, 0, -2]) and not ok([8] * 5)
    assert host.prp_host_check_plane(None, 1) == 1 and host.prp_host_check_plane(None, 0) == 0 and host.prp_host_check_plane(None, -1) == 1


def test_ground_truth_conditions(host):
    """Conditions, not measurements; the figures are recorded in profiles/pose_refine_plane.txt."""
    g = prc.ground_truth_case()
    nrm = ppc.ground_truth_normals()
    assert int((nrm[..., 3] != 0).sum()) >= int((g["scene"] != 0).sum()) - 8
    errors = lambda rec: prc.pose_errors(*prc.compose(g["R_a"], g["distance"], rec), g["R_b"], g["T_b_m"])
    for (x, y) in ppc.ground_truth_placements():
        P = prc.make_params(prc.GT_CAM, prc.GT_CAM, max_iterations=ppc.GT_ITERATIONS)
        rec, _, plane, trace = _both(host, P, None, [ppc.GT_SHIFT], g["crop"], g["rect"][:2], g["scene"], nrm, x, y, ("ground truth", x, y))
        err = errors(rec)
        point, _ = ppc.host_refine_point(host, P, g["crop"], g["rect"][:2], g["scene"], x, y, POSE_REFINE_DTYPE)
        placed, _ = ppc.host_refine_point(host, dict(P, max_iterations=0), g["crop"], g["rect"][:2], g["scene"], x, y, POSE_REFINE_DTYPE)
        e_point, e_placed = errors(point[0]), errors(placed[0])
        print("match (%d, %d): plane shift %d, %d iterations: status %d, rms %.4f -> %.4f mm, %.4f deg %.4f mm; point-to-point, %d iterations: %.4f deg %.4f mm; "
              "placement: %.4f deg %.4f mm" % (x, y, ppc.GT_SHIFT, rec["iterations"], rec["status"], rec["rms_first_mm"], rec["rms_last_mm"], err[0], err[1],
                                               ppc.GT_ITERATIONS, e_point[0], e_point[1], e_placed[0], e_placed[1]))
        assert all(r == ppc.PLANE for _, _, r in trace[:-1]) and plane[0, 0] > 0
        assert rec["status"] in (prc.CONVERGED, prc.MAX_ITERATIONS)
        assert rec["rms_last_mm"] < rec["rms_first_mm"]
        assert err[0] < e_placed[0] and err[1] < e_placed[1], (err, e_placed)
        assert err[0] <= e_point[0] and err[1] <= e_point[1], (err, e_point)


def test_border_cases_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "pose_refine_plane_host")
    subprocess.check_call(["g++"] + ppc.HOST_FLAGS + san + [ppc.HOST_SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "pose_refine_plane_host ok" in res.stdout


def test_the_setter_without_a_device():
    """The setting lives on the host: setting, reading and refusing it touch no device."""
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16)])                            # no pixel: enable_normals needs no device either
    assert t.get_refine_plane() == []
    t.set_refine_plane([-1, -1])                                                              # no entry reads a normal: admitted before enable_normals
    assert t.get_refine_plane() == [-1, -1]
    with pytest.raises(_lib.LmxError) as e:
        t.set_refine_plane([-1, 8])
    assert e.value.status == INV and "enable_normals" in str(e.value)
    assert t.get_refine_plane() == [-1, -1]                                                   # the previous setting stays
    t.enable_normals(400.0, 400.0)
    t.set_refine_plane([8, -1, 0, 20])
    assert t.get_refine_plane() == [8, -1, 0, 20]
    for bad in ([21], [-2], [8, 8, 8, 8, 8], [0, 0, 0, 33]):
        with pytest.raises(_lib.LmxError) as e:
            t.set_refine_plane(bad)
        assert e.value.status == INV
        assert t.get_refine_plane() == [8, -1, 0, 20], bad
    arr = (C.c_int32 * 4)(8, 8, 8, 8)
    n = C.c_int32(0)
    assert L.lmx_depth_templates_set_refine_plane(None, arr, 1) == INV and b"null" in L.lmx_last_error()
    assert L.lmx_depth_templates_set_refine_plane(t.h, None, 1) == INV and b"null" in L.lmx_last_error()
    assert L.lmx_depth_templates_set_refine_plane(t.h, arr, 5) == INV and L.lmx_depth_templates_set_refine_plane(t.h, arr, -1) == INV
    assert t.get_refine_plane() == [8, -1, 0, 20]
    assert L.lmx_depth_templates_get_refine_plane(t.h, None, C.byref(n)) == INV and L.lmx_depth_templates_get_refine_plane(None, arr, C.byref(n)) == INV
    assert L.lmx_depth_templates_get_refine_plane(t.h, arr, None) == INV
    assert L.lmx_depth_templates_set_refine_plane(t.h, arr, 1) == _lib.LMX_OK
    assert L.lmx_depth_templates_get_refine_plane(t.h, arr, C.byref(n)) == _lib.LMX_OK and n.value == 1 and list(arr) == [8, -1, -1, -1]
    t.set_refine_plane(None)
    assert t.get_refine_plane() == []
    t.set_refine_plane([4])
    t.set_refine_plane([])
    assert t.get_refine_plane() == []
    assert L.lmx_depth_templates_set_refine_plane(t.h, arr, 0) == _lib.LMX_OK and t.get_refine_plane() == []   # n_stages 0 clears, whatever the pointer
    t.close()
