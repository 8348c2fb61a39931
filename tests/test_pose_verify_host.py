"""Pose verification without a device: the shared header (csrc/lmx_pose_verify.hpp, built with plain g++ from tests/cpp/pose_verify_host.cpp)
against the numpy restatement of tests/pose_verify_cases.py in every byte of every record; the exact properties the constructed jobs
were built for; the keep rule from Python, from the header and from the library; the refusals of parameters and poses; the same C++
file's main() under AddressSanitizer + UBSan as a child process; the argument checks of the new entry points."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pose_refine_cases as prc
import pose_verify_cases as pvc
from conftest import has_gpu
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE, DepthTemplates, keep_verified


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pvc.build_host(tmp_path_factory.mktemp("pvhost"))


@pytest.fixture(scope="module")
def records(host):
    """Every constructed job through the restatement and the header, equal in every byte -> {name: (job, record dict)}."""
    out = {}
    for j in pvc.constructed_jobs():
        rec = pvc.np_verify(j.P, j.crop, j.rect_xy, j.scene, j.R, j.t)
        got = pvc.host_verify(host, j.P, j.crop, j.rect_xy, j.scene, j.R, j.t, POSE_VERIFY_DTYPE)
        want = pvc.record_array(rec, POSE_VERIFY_DTYPE)
        for k in POSE_VERIFY_DTYPE.names:
            assert want[k].tobytes() == got[k].tobytes(), (j.name, k, want[k], got[k])
        assert want.tobytes() == got.tobytes(), j.name
        out[j.name] = (j, rec)
    return out


def test_record_layout():
    assert POSE_VERIFY_DTYPE.itemsize == 48 and POSE_VERIFY_DTYPE.itemsize % 8 == 0
    assert [POSE_VERIFY_DTYPE.fields[k][1] for k in ("rate", "n_model", "status", "roi")] == [0, 8, 28, 32]
    assert C.sizeof(_lib.PoseVerifyParams) == 96


def test_header_equals_the_numpy_restatement(records):
    assert {r["status"] for _, r in records.values()} == {pvc.OK, pvc.EMPTY, pvc.GRID_TOO_LARGE}
    for name, (j, r) in records.items():
        assert r["n_model"] == int((j.crop != 0).sum()), name
        assert 0 <= r["n_occupied"] <= r["n_tested"] <= r["n_model"], name


def test_exact_properties_of_the_constructed_jobs(records):
    sizes = {name: r["n_model"] for name, (_, r) in records.items()}
    assert sizes["identity_1x1"] == 1 and sizes["identity_17x1"] == 17 and sizes["identity_70x70"] > 256 * 16     # a lane walks several vectors
    for name, (j, r) in records.items():
        if j.expect == "all":        # every model point meets its own scene point
            assert r["status"] == pvc.OK and r["rate"] == 1.0 and r["n_occupied"] == r["n_tested"] == r["n_model"] > 0, (name, r)
            assert r["n_scene"] >= r["n_model"], name
        elif j.expect == "none":
            assert r["status"] == pvc.OK and r["n_occupied"] == 0 and r["rate"] == 0.0 and r["n_tested"] == r["n_model"], (name, r)
        elif j.expect == "outside":
            assert r["status"] == pvc.OK and r["n_scene"] == 0 and r["n_occupied"] == 0 and r["rate"] == 0.0 and r["roi"] == [0, 0, 0, 0], (name, r)
            assert r["n_tested"] == r["n_model"] > 0 and r["cells"] > 0, name
        elif j.expect == "clipped":
            x, y, w, h = r["roi"]
            on_image = 0 < w < 33 + 16 and 0 < h < 37 + 16 and (x == 0 or x + w == pvc.SCENE_W) and (y == 0 or y + h == pvc.SCENE_H)
            assert r["status"] == pvc.OK and on_image and 0 < r["n_occupied"] < r["n_model"], (name, r)
        elif j.expect in (pvc.EMPTY, pvc.GRID_TOO_LARGE):
            assert r["status"] == j.expect and r["n_occupied"] == 0 and r["n_scene"] == 0 and r["rate"] == 0.0, (name, r)
    # the occluder: what it leaves uncovered still meets its own scene points
    j, r = records["left_half_occluded"]
    uncovered = int((j.crop[:, 16:] != 0).sum())
    assert uncovered / r["n_model"] <= r["rate"] < 1.0 and r["n_occupied"] >= uncovered, r
    # keys left of and above the principal point are negative, and flooring them is not truncating them
    j, r = records["straddles_principal_point"]
    _, K, _, _, T = pvc.np_model_points(j.P, j.crop, j.rect_xy, j.R, j.t)
    vt = 64
    assert (K[:, 0] < 0).any() and (K[:, 1] < 0).any() and (K[:, 0] > 0).any()
    trunc = np.sign(T) * (np.abs(T) // vt)
    assert (trunc != K).any() and ((T < 0) & (T % vt != 0)).any()
    # the margin decides which scene pixels are seen when the pose is off by three pixels
    (_, r0), (_, r8) = records["shifted_margin_0"], records["shifted_margin_8"]
    assert r0 != r8 and r0["n_scene"] < r8["n_scene"] and r0["roi"][2] + 16 == r8["roi"][2]
    # the refined pose of the turned object explains the scene, the unrefined one does not
    rec = pvc.turned_case()[3]
    R = np.asarray(rec["R"]).reshape(3, 3)
    angle = np.degrees(np.arccos((np.trace(R) - 1.0) / 2.0))
    assert rec["status"] in (prc.CONVERGED, prc.MAX_ITERATIONS) and 8.0 < angle < 12.0 and abs(R[0, 2]) > 0.12, (angle, R)
    assert records["turned_by_refine"][1]["rate"] > 0.8 > records["turned_identity"][1]["rate"]
    # the cap: 2^17 < cells <= 2^18 runs, the first size above it does not
    assert 2 ** 17 < records["cap_below"][1]["cells"] <= pvc.MAX_CELLS < records["cap_above"][1]["cells"] < pvc.MAX_CELLS + 2 ** 11
    assert records["cap_above"][1]["roi"][2] > 0
    assert records["voxel_64"][1]["cells"] <= 27 and 0 < records["voxel_64_behind"][1]["n_occupied"] < records["voxel_64_behind"][1]["n_model"]


def test_keep_rule_from_python_the_header_and_the_library(records, host):
    recs = [r for _, r in records.values()]
    arr = np.concatenate([pvc.record_array(r, POSE_VERIFY_DTYPE) for r in recs] + [np.zeros(1, POSE_VERIFY_DTYPE)])
    recs.append(dict(status=pvc.NONE, rate=0.0))
    rate = records["left_half_occluded"][1]["rate"]
    L = _lib.lib()
    for thresh in (0.3, 0.2, 0.0, 1.0, rate, np.nextafter(rate, 1.0), np.nextafter(rate, 0.0), float("nan"), float("inf"), -1.0):
        want = pvc.np_keep(recs, thresh)
        got_py = keep_verified(arr, thresh)
        got_h, got_l = np.full(len(arr), 7, np.uint8), np.full(len(arr), 7, np.uint8)
        host.pv_host_keep(arr.ctypes.data, len(arr), thresh, got_h.ctypes.data)
        assert L.lmx_pose_verify_keep(arr.ctypes.data, len(arr), thresh, got_l.ctypes.data) == _lib.LMX_OK
        assert got_py.dtype == bool and got_py.tolist() == want.tolist() == got_h.astype(bool).tolist() == got_l.astype(bool).tolist(), thresh
        assert set(got_l.tolist()) <= {0, 1}
    k = list(records).index("left_half_occluded")
    assert keep_verified(arr, rate)[k] and not keep_verified(arr, np.nextafter(rate, 1.0))[k]         # rate == thresh keeps
    nan_keeps = keep_verified(arr, float("nan"))
    assert nan_keeps.tolist() == (arr["status"] == pvc.OK).tolist() and not nan_keeps[-1]               # a NaN threshold erases nothing that ran
    assert L.lmx_pose_verify_keep(None, 0, 0.3, None) == _lib.LMX_OK
    assert L.lmx_pose_verify_keep(None, 1, 0.3, got_l.ctypes.data) == _lib.LMX_ERR_INVALID_ARG and b"null" in L.lmx_last_error()
    assert L.lmx_pose_verify_keep(arr.ctypes.data, 1, 0.3, None) == _lib.LMX_ERR_INVALID_ARG


def test_header_refuses_parameters_and_poses_out_of_range(host):
    c, r = pvc.make_crop(8, 8, (30, 20))
    scene = pvc.paste(c, r)
    nan, inf = float("nan"), float("inf")

    def rc(R=pvc.IDENTITY, t=(0.0, 0.0, 0.0), **kw):
        return pvc.host_verify_rc(host, pvc.make_params(**kw), c, r, scene, R, t, POSE_VERIFY_DTYPE)[0]

    assert rc() == 0 and rc(voxel_mm=0.25, roi_margin=0) == 0 and rc(voxel_mm=64.0, roi_margin=64) == 0
    for bad in (dict(voxel_mm=0.2499), dict(voxel_mm=64.5), dict(voxel_mm=nan), dict(voxel_mm=-4.0), dict(roi_margin=-1), dict(roi_margin=65),
                dict(model=(0.0, 400.0, 48.0, 40.0)), dict(scene=(400.0, nan, 48.0, 40.0)), dict(scene=(400.0, 400.0, 2.0 ** 21, 40.0))):
        assert rc(**bad) == 1, bad
    for k in range(9):
        for v in (nan, inf, -inf, 2.0000001, -2.5):
            R = list(pvc.IDENTITY)
            R[k] = v
            assert rc(R=R) == 2, (k, v)
    for k in range(3):
        for v in (nan, inf, 2.0 ** 20 + 1.0, -2.0 ** 20 - 1.0):
            t = [0.0, 0.0, 0.0]
            t[k] = v
            assert rc(t=t) == 2, (k, v)
    assert rc(R=[2.0, -2.0, 2.0, -2.0, 2.0, -2.0, 2.0, -2.0, 2.0], t=(2.0 ** 20, -2.0 ** 20, 2.0 ** 20)) == 0


def test_border_poses_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "pose_verify_host")
    subprocess.check_call(["g++"] + pvc.HOST_FLAGS + san + [pvc.HOST_SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "pose_verify_host ok" in res.stdout


# ---- argument checks (no device needed up to the point where LMX_ERR_NO_DEVICE is the answer) ------------------------------------------

def _image(a, channels=1, elem_size=2):
    return _lib.Image(a.ctypes.data, a.shape[0], a.shape[1], channels, elem_size, a.strides[0])


def _params(**kw):
    v = dict(struct_size=C.sizeof(_lib.PoseVerifyParams), model_fx=400.0, model_fy=400.0, model_cx=8.0, model_cy=6.0, scene_fx=400.0, scene_fy=400.0, scene_cx=8.0,
             scene_cy=6.0, voxel_mm=4.0, roi_margin=8, rects=None)
    v.update(kw)
    return _lib.PoseVerifyParams(**v)


def _poses(n):
    p = np.zeros(n, POSE_REFINE_DTYPE)
    p["R"][:] = pvc.IDENTITY
    p["status"] = prc.CONVERGED
    return p


def test_pose_verify_argument_checks():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16), np.zeros((0, 0), np.uint16)])   # two empty templates: no device touched
    d0, d1 = np.ones((12, 16), np.uint16), np.ones((12, 16), np.uint16)
    m = np.zeros(3, MATCH_DTYPE)
    out = np.full(3, 7, POSE_VERIFY_DTYPE).view(np.uint8)
    out[:] = 7
    good, ok_poses = _params(), _poses(3)

    def verify(h=t.h, imgs=(d0, d1), images=None, nf=2, matches=m, offsets=(0, 1, 3), cls=-1, poses=ok_poses, p=good, o=out):
        arr = images if images is not None else ((_lib.Image * len(imgs))(*[_image(a) for a in imgs]) if imgs is not None else None)
        offs = (C.c_size_t * len(offsets))(*offsets) if offsets is not None else None
        return L.lmx_pose_verify_matches(h, arr, nf, matches.ctypes.data if matches is not None else None, offs, cls, poses.ctypes.data if poses is not None else None,
                                         C.byref(p) if p is not None else None, o.ctypes.data if o is not None else None)

    assert verify(h=None) == INV and b"null" in L.lmx_last_error()
    assert verify(p=None) == INV and verify(offsets=None) == INV and verify(matches=None) == INV and verify(o=None) == INV and verify(poses=None) == INV
    assert verify(p=_params(struct_size=8)) == INV and b"struct_size" in L.lmx_last_error()
    nan = float("nan")
    for bad in (dict(model_fx=0.0), dict(scene_fy=nan), dict(scene_fx=float("inf")), dict(model_cx=nan), dict(scene_cy=2.0 ** 21), dict(voxel_mm=0.0), dict(voxel_mm=0.24),
                dict(voxel_mm=65.0), dict(voxel_mm=nan), dict(roi_margin=-1), dict(roi_margin=65)):
        assert verify(p=_params(**bad)) == INV, bad
    assert b"roi_margin" in L.lmx_last_error()
    assert verify(p=_params(voxel_mm=100.0)) == INV and b"voxel_mm" in L.lmx_last_error()
    assert verify(nf=-1) == INV and b"n_frames" in L.lmx_last_error()
    assert verify(offsets=(1, 1, 3)) == INV and verify(offsets=(0, 2, 1)) == INV and b"offsets" in L.lmx_last_error()
    assert verify(images=(_lib.Image * 2)(_image(d0), _image(d1, elem_size=4))) == _lib.LMX_ERR_SHAPE
    assert verify(imgs=(d0, np.ones((12, 17), np.uint16))) == _lib.LMX_ERR_SHAPE
    assert verify(imgs=None) == INV and b"no scene is uploaded" in L.lmx_last_error()
    bad = m.copy()
    bad["template_id"][2] = 2
    assert verify(matches=bad) == INV and b"match 2" in L.lmx_last_error() and b"template_id 2" in L.lmx_last_error()
    # poses: refused with the match's index, before any device work, unless the match is not selected
    for field, k, v, word in (("R", 4, nan, b"R"), ("R", 0, 2.5, b"R"), ("R", 8, float("-inf"), b"R"), ("t_mm", 1, 2.0 ** 20 + 1.0, b"t_mm"), ("t_mm", 2, nan, b"t_mm")):
        pp = ok_poses.copy()
        pp[field][1, k] = v
        assert verify(poses=pp) == INV and b"match 1:" in L.lmx_last_error() and word in L.lmx_last_error(), (field, k, v)
        after = _lib.LMX_OK if has_gpu() else _lib.LMX_ERR_NO_DEVICE     # the other two matches are valid ones of (empty) templates
        cl = m.copy()
        cl["class_index"][1] = 3                       # another class's match: its pose is not looked at
        assert verify(poses=pp, matches=cl, cls=0) == after
        pp["status"][1] = prc.NONE                     # not refined: neither
        assert verify(poses=pp) == after
    none = ok_poses.copy()
    none["status"] = prc.NONE
    none["R"][:, 0] = nan
    assert verify(poses=none) == _lib.LMX_OK and not out.any()       # nothing selected: zeros, no device
    out[:] = 7
    cl = m.copy()
    cl["class_index"][:] = 1
    assert verify(matches=cl, cls=0, poses=none) == _lib.LMX_OK and not out.any()
    out[:] = 7
    assert verify(nf=0, imgs=None, offsets=None, matches=None, o=None, poses=None) == _lib.LMX_OK
    assert verify(offsets=(0, 0, 0), matches=None, o=None, poses=None) == _lib.LMX_OK and (out == 7).all()
    if not has_gpu():
        assert verify() == _lib.LMX_ERR_NO_DEVICE      # valid matches of (empty) templates need the device
    # the Python front end's own refusals
    with pytest.raises(ValueError):
        t.verify_poses(m, ok_poses, d0)                                           # no cameras
    with pytest.raises(ValueError):
        t.verify_poses(m, ok_poses[:2], d0, model_camera=prc.CAM, scene_camera=prc.CAM)
    with pytest.raises(ValueError):
        t.verify_poses(m, ok_poses, [d0, d1], model_camera=prc.CAM, scene_camera=prc.CAM)   # two frames, no offsets
    with pytest.raises(ValueError):
        t.verify_poses(m, ok_poses, d0, model_camera=prc.CAM, scene_camera=prc.CAM, rects=np.zeros((3, 4), np.int32))
    with pytest.raises(_lib.LmxError) as e:
        t.verify_poses(m, ok_poses, None, model_camera=prc.CAM, scene_camera=prc.CAM)
    assert e.value.status == INV
    with pytest.raises(_lib.LmxError) as e:
        t.verify_poses(m, ok_poses, d0, model_camera=prc.CAM, scene_camera=prc.CAM, voxel_mm=0.1)
    assert e.value.status == INV and "voxel_mm" in str(e.value)
    t.close()
