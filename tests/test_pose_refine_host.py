"""Pose refinement without a device: the shared header (csrc/lmx_pose_refine.hpp, built with plain g++ from tests/cpp/pose_refine_host.cpp)
against the numpy restatement of tests/pose_refine_cases.py -- the integer sums of every pass and every byte of the record; the
ground-truth case (a golden mesh rendered at two poses); lmx_pose_compose against numpy; the same C++ file's main() under
AddressSanitizer + UBSan as a child process; the argument checks of the new entry points."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pose_refine_cases as prc
from conftest import has_gpu
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, DepthTemplates, cluster_leaders, compose_pose
from linemod_pose_estimation_amd.detector import CLUSTER_DTYPE


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return prc.build_host(tmp_path_factory.mktemp("prhost"))


def _both(host, P, crop, rect_xy, scene, x, y, what):
    """The restatement and the header on one job, equal in every sum and every byte -> (record dict, sums)."""
    rec, sums = prc.np_refine(P, crop, rect_xy, scene, x, y)
    got, got_sums = prc.host_refine(host, P, crop, rect_xy, scene, x, y, POSE_REFINE_DTYPE)
    assert np.array_equal(sums, got_sums), what
    want = prc.record_array(rec, POSE_REFINE_DTYPE)
    for k in POSE_REFINE_DTYPE.names:
        assert want[k].tobytes() == got[k].tobytes(), (what, k, want[k], got[k])
    assert want.tobytes() == got.tobytes(), what
    return rec, sums


def test_header_equals_the_numpy_restatement(host):
    scenes = prc.scenes()
    seen, by_name = set(), {}
    for j in prc.constructed_jobs():
        rec, sums = _both(host, j.P, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, j.name)
        if j.expect is not None:
            assert rec["status"] == j.expect, (j.name, rec["status"])
        assert rec["n_model"] == int((j.crop != 0).sum())
        assert not sums[rec["iterations"] + 1:].any() and (rec["status"] == prc.NO_OVERLAP or sums[rec["iterations"], 0] == rec["n_pairs_last"])
        seen.add(rec["status"])
        by_name[j.name] = (rec, sums)
    assert seen == {prc.CONVERGED, prc.MAX_ITERATIONS, prc.NO_OVERLAP, prc.LOST}
    # LOST in a later pass, with the pose of the step before it
    rec, sums = by_name["lost_later"]
    assert rec["iterations"] >= 1 and sums[0, 0] >= 27 > sums[rec["iterations"], 0] and rec["R"] != [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    # the singular system: the first pivot is 0 exactly, the step is translation-only
    rec, sums = by_name["singular_row"]
    assert sums[0, 0] == 24 and sums[0, 10] + sums[0, 12] == 0 and rec["R"] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and rec["iterations"] >= 1
    assert rec["t_mm"][2] == -5.0
    # the window matters over holes, and the iteration limits are what they say
    assert not np.array_equal(by_name["radius_0_border"][1][0], by_name["radius_1_border"][1][0])
    assert not np.array_equal(by_name["radius_1_far_border"][1][0], by_name["radius_2_far_border"][1][0])
    assert [by_name["iterations_%d" % n][0]["iterations"] for n in (0, 1, 64)] == [0, 1, 64]
    r0 = by_name["iterations_0"][0]
    assert r0["rms_first_mm"] == r0["rms_last_mm"] > 0 and r0["R"] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def test_header_refuses_parameters_out_of_range(host):
    c, r = prc.make_crop(8, 8, (30, 20))
    scene = prc.make_scene()
    pad = np.zeros((8, 8), np.uint16)
    pad[:] = c
    rec = np.zeros(1, POSE_REFINE_DTYPE)
    good = prc.make_params(prc.CAM, prc.CAM)

    def refused(**kw):
        P = dict(good, **kw)
        v = prc.params_vector(P)
        return host.pr_host_refine(pad.ctypes.data, 8, 8, 8, r[0], r[1], scene.ctypes.data, prc.SCENE_W, prc.SCENE_H, prc.SCENE_W, 30, 20, v.ctypes.data,
                                   rec.ctypes.data, None)

    assert refused() == 0
    nan = float("nan")
    for bad in (dict(model=(0.0, 400.0, 48.0, 40.0)), dict(model=(400.0, -1.0, 48.0, 40.0)), dict(scene=(nan, 400.0, 48.0, 40.0)), dict(scene=(400.0, 400.0, nan, 40.0)),
                dict(scene=(400.0, 2.0 ** 21, 48.0, 40.0)), dict(max_dist_mm=0.0), dict(max_dist_mm=1024.5), dict(max_dist_mm=nan), dict(eps_rot_rad=-1e-9),
                dict(eps_trans_mm=nan), dict(max_iterations=-1), dict(max_iterations=65), dict(min_pairs=2), dict(search_radius=-1), dict(search_radius=3)):
        assert refused(**bad) == 1, bad
    assert refused(max_dist_mm=1024.0, max_iterations=64, min_pairs=3, search_radius=2, eps_rot_rad=0.0) == 0


def test_ground_truth_two_renders_of_a_golden_mesh(host):
    """Conditions, not measurements; the figures the restatement gets are recorded in profiles/pose_refine.txt."""
    g = prc.ground_truth_case()
    assert g["scene"].shape == (240, 320) and int((g["crop"] != 0).sum()) >= 400
    bx, by = g["rect_b"][:2]
    for (x, y) in ((bx, by), (bx + 1, by), (bx, by + 1)):
        errs = {}
        for it in (0, 20):
            P = prc.make_params(prc.GT_CAM, prc.GT_CAM, max_iterations=it)
            rec, _ = _both(host, P, g["crop"], g["rect"][:2], g["scene"], x, y, ("ground truth", x, y, it))
            R_obj, t_obj = prc.compose(g["R_a"], g["distance"], rec)
            errs[it] = prc.pose_errors(R_obj, t_obj, g["R_b"], g["T_b_m"])
            print("match (%d, %d), max_iterations %d: status %d after %d iterations, rms %.4f -> %.4f mm, rotation error %.4f deg, translation error %.4f mm"
                  % (x, y, it, rec["status"], rec["iterations"], rec["rms_first_mm"], rec["rms_last_mm"], errs[it][0], errs[it][1]))
        assert rec["status"] in (prc.CONVERGED, prc.MAX_ITERATIONS)
        assert rec["rms_last_mm"] < rec["rms_first_mm"]
        assert errs[20][0] < errs[0][0] and errs[20][1] < errs[0][1], errs
    # the same render as template and scene: nothing to move, and one iteration says so
    P = prc.make_params(prc.GT_CAM, prc.GT_CAM)
    rec, _ = _both(host, P, g["crop"], g["rect"][:2], g["scene_a"], g["rect"][0], g["rect"][1], "identical")
    R = np.asarray(rec["R"]).reshape(3, 3)
    angle = np.arccos(min(1.0, (np.trace(R) - 1.0) / 2.0))
    assert rec["status"] == prc.CONVERGED and rec["iterations"] == 1
    assert angle <= P["eps_rot_rad"] and np.linalg.norm(rec["t_mm"]) <= P["eps_trans_mm"]


def test_pose_compose_equals_numpy():
    rng = np.random.RandomState(3)
    L = _lib.lib()
    for _ in range(5):
        q = rng.randn(4)
        q /= np.linalg.norm(q)
        rec = dict(R=prc._rotation_of(list(q)), t_mm=list(rng.randn(3) * 20.0))
        qa = rng.randn(4)
        qa /= np.linalg.norm(qa)
        view = (np.asarray(prc._rotation_of(list(qa))).reshape(3, 3), 0.4 + rng.rand() * 0.3)
        r = np.zeros(1, POSE_REFINE_DTYPE)
        r["R"][0], r["t_mm"][0] = rec["R"], rec["t_mm"]
        R_obj, t_obj = compose_pose(view, r[0])
        want_R, want_t = prc.compose(view[0], view[1], rec)
        assert R_obj.tobytes() == want_R.tobytes() and t_obj.tobytes() == want_t.tobytes()
        assert np.allclose(R_obj, np.asarray(rec["R"]).reshape(3, 3) @ view[0], atol=1e-14)
        assert np.allclose(t_obj * 1000.0, np.asarray(rec["R"]).reshape(3, 3) @ [0, 0, 1000.0 * view[1]] + rec["t_mm"], atol=1e-10)
    v = _lib.MeshView((C.c_double * 9)(*([1, 0, 0, 0, 1, 0, 0, 0, 1])), 0.5)
    out9, out3 = np.zeros(9), np.zeros(3)
    INV = _lib.LMX_ERR_INVALID_ARG
    assert L.lmx_pose_compose(None, r.ctypes.data, out9.ctypes.data, out3.ctypes.data) == INV and b"null" in L.lmx_last_error()
    assert L.lmx_pose_compose(C.byref(v), None, out9.ctypes.data, out3.ctypes.data) == INV
    assert L.lmx_pose_compose(C.byref(v), r.ctypes.data, None, out3.ctypes.data) == INV
    assert L.lmx_pose_compose(C.byref(v), r.ctypes.data, out9.ctypes.data, None) == INV


def test_cluster_leaders():
    m = np.zeros(7, MATCH_DTYPE)
    m["similarity"] = [80, 95, 95, 70, 60, 99, 60]
    members = np.asarray([3, 2, 1, 0, 6, 4, 5], np.int32)
    cl = np.zeros(3, CLUSTER_DTYPE)
    cl["member_begin"], cl["member_count"] = [0, 4, 6], [4, 2, 1]
    assert cluster_leaders(cl, members, m).tolist() == [2, 6, 5]      # 2 before 1 (both 95) and 6 before 4 (both 60): the first in member order
    assert cluster_leaders(cl[:0], members, m).tolist() == []
    cl["member_count"][1] = 0
    with pytest.raises(ValueError):
        cluster_leaders(cl, members, m)


def test_border_cases_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "pose_refine_host")
    subprocess.check_call(["g++"] + prc.HOST_FLAGS + san + [prc.HOST_SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "pose_refine_host ok" in res.stdout


# ---- argument checks (no device needed up to the point where LMX_ERR_NO_DEVICE is the answer) ------------------------------------------

def _image(a, channels=1, elem_size=2):
    return _lib.Image(a.ctypes.data, a.shape[0], a.shape[1], channels, elem_size, a.strides[0])


def _params(**kw):
    v = dict(struct_size=C.sizeof(_lib.PoseRefineParams), model_fx=400.0, model_fy=400.0, model_cx=8.0, model_cy=6.0, scene_fx=400.0, scene_fy=400.0, scene_cx=8.0,
             scene_cy=6.0, max_dist_mm=10.0, eps_rot_rad=1e-5, eps_trans_mm=1e-3, max_iterations=20, min_pairs=16, search_radius=1, rects=None)
    v.update(kw)
    return _lib.PoseRefineParams(**v)


def test_pose_refine_argument_checks():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16), np.zeros((0, 0), np.uint16)])   # two empty templates: no device touched
    d0, d1 = np.ones((12, 16), np.uint16), np.ones((12, 16), np.uint16)
    m = np.zeros(3, MATCH_DTYPE)
    out = np.full(3, 7, POSE_REFINE_DTYPE).view(np.uint8)
    out[:] = 7
    good = _params()

    def refine(h=t.h, imgs=(d0, d1), images=None, nf=2, matches=m, offsets=(0, 1, 3), cls=-1, p=good, o=out):
        arr = images if images is not None else ((_lib.Image * len(imgs))(*[_image(a) for a in imgs]) if imgs is not None else None)
        offs = (C.c_size_t * len(offsets))(*offsets) if offsets is not None else None
        return L.lmx_pose_refine_matches(h, arr, nf, matches.ctypes.data if matches is not None else None, offs, cls, C.byref(p) if p is not None else None,
                                         o.ctypes.data if o is not None else None)

    assert refine(h=None) == INV and b"null" in L.lmx_last_error()
    assert refine(p=None) == INV and refine(offsets=None) == INV and refine(matches=None) == INV and refine(o=None) == INV
    assert refine(p=_params(struct_size=8)) == INV and b"struct_size" in L.lmx_last_error()
    nan = float("nan")
    for bad in (dict(model_fx=0.0), dict(model_fy=-3.0), dict(scene_fx=nan), dict(scene_fy=nan), dict(scene_fx=float("inf")), dict(model_cx=nan), dict(scene_cy=2.0 ** 21),
                dict(max_dist_mm=0.0), dict(max_dist_mm=2000.0), dict(max_dist_mm=nan), dict(eps_rot_rad=-1.0), dict(eps_trans_mm=nan), dict(max_iterations=-1),
                dict(max_iterations=65), dict(min_pairs=2), dict(search_radius=3), dict(search_radius=-1)):
        assert refine(p=_params(**bad)) == INV, bad
    assert b"search_radius" in L.lmx_last_error()
    assert refine(p=_params(model_fx=nan)) == INV and b"focal" in L.lmx_last_error()
    assert refine(nf=-1) == INV and b"n_frames" in L.lmx_last_error()
    assert refine(offsets=(1, 1, 3)) == INV and refine(offsets=(0, 2, 1)) == INV and b"offsets" in L.lmx_last_error()
    assert refine(images=(_lib.Image * 2)(_image(d0), _image(d1, elem_size=4))) == _lib.LMX_ERR_SHAPE
    assert refine(imgs=(d0, np.ones((12, 17), np.uint16))) == _lib.LMX_ERR_SHAPE and b"image 1 is 17 x 12" in L.lmx_last_error()
    assert refine(images=(_lib.Image * 2)(_image(d0), _lib.Image(None, 12, 16, 1, 2, 32))) == INV
    # depth == NULL: the resident scene, and there is none
    assert refine(imgs=None) == INV and b"no scene is uploaded" in L.lmx_last_error()
    bad = m.copy()
    bad["template_id"][2] = 2
    assert refine(matches=bad) == INV and b"match 2" in L.lmx_last_error() and b"template_id 2" in L.lmx_last_error()
    bad["template_id"][2] = -1
    assert refine(matches=bad) == INV and b"match 2" in L.lmx_last_error()
    far = np.asarray([[0, 0, 0, 0], [1 << 17, 0, 0, 0]], np.int32)
    far[1, 0] += 1
    one = m.copy()
    one["template_id"][1] = 1
    assert refine(matches=one, p=_params(rects=far.ctypes.data)) == INV and b"match 1" in L.lmx_last_error() and b"rect" in L.lmx_last_error()
    bad["class_index"][2] = 4                 # another class's match: its template id is not this object's to judge
    bad["class_index"][:2] = 1
    assert refine(matches=bad, cls=0) == _lib.LMX_OK and not out.any()       # nothing selected: zeros, no device
    out[:] = 7
    assert refine(nf=0, imgs=None, offsets=None, matches=None, o=None) == _lib.LMX_OK
    assert refine(offsets=(0, 0, 0), matches=None, o=None) == _lib.LMX_OK and (out == 7).all()
    # the test hook
    sums = np.zeros((21, 17), np.int64)
    img = (_lib.Image * 1)(_image(d0))
    hook = lambda h=t.h, i=img, mm=m.ctypes.data, p=good, o=out.ctypes.data, s=sums.ctypes.data: L.lmx_debug_pose_refine_sums(h, i, mm, C.byref(p) if p is not None else None, o, s)
    assert hook(h=None) == INV and hook(i=None) == INV and hook(mm=None) == INV and hook(p=None) == INV and hook(o=None) == INV and hook(s=None) == INV
    assert hook(p=_params(max_iterations=65)) == INV
    if not has_gpu():
        assert refine() == _lib.LMX_ERR_NO_DEVICE      # valid matches of (empty) templates need the device
        assert hook() == _lib.LMX_ERR_NO_DEVICE
    # the Python front end's own refusals
    with pytest.raises(ValueError):
        t.refine_poses(m, d0)                                           # no cameras
    with pytest.raises(ValueError):
        t.refine_poses(m, [d0, d1], model_camera=prc.CAM, scene_camera=prc.CAM)   # two frames, no offsets
    with pytest.raises(ValueError):
        t.refine_poses(m, d0, model_camera=prc.CAM, scene_camera=prc.CAM, rects=np.zeros((3, 4), np.int32))
    with pytest.raises(_lib.LmxError) as e:
        t.refine_poses(m, None, model_camera=prc.CAM, scene_camera=prc.CAM)
    assert e.value.status == INV
    t.close()
