"""The mesh rasteriser's device header on the CPU (tests/cpp/mesh_raster_host.cpp: linemod_pose_estimation_amd/csrc/lmx_mesh_raster.hpp
compiled with LMX_MR_HOST, -ffp-contract=off) against meshsynth.render_view (meshraster.c), every byte of gray, depth, mask and rect; and
the argument checks of the two entry points built on it (lmx_mesh_render, lmx_bank_train_mesh).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
from conftest import ROOT, has_gpu
from linemod_pose_estimation_amd import _lib, meshsynth as ms, NativeBank

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")


@pytest.fixture(scope="module")
def mr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mrhost") / "libmrhost.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "mesh_raster_host.cpp")])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.mr_host_render.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, C.c_int, vp, vp, vp, vp]
    return lib


def host_render(lib, tri, cam, views, fill=0x5a):
    tri = np.ascontiguousarray(tri, np.float64)
    n, H, W = len(views), cam["height"], cam["width"]
    pv = mc.pack_views(views)
    light = np.asarray(mc.LIGHT, np.float64)
    gray = np.full((n, H, W), fill, np.uint8)
    depth = np.full((n, H, W), fill, np.uint16)
    mask = np.full((n, H, W), fill, np.uint8)
    rects = np.full((n, 4), -7, np.int32)
    rc = lib.mr_host_render(tri.ctypes.data, len(tri), W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], light.ctypes.data, pv.ctypes.data, n,
                            gray.ctypes.data, depth.ctypes.data, mask.ctypes.data, rects.ctypes.data)
    return rc, gray, depth, mask, rects


CASES = mc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_header_equals_meshraster_c(mr, case):
    name, tri, cam, views = case
    rc, gray, depth, mask, rects = host_render(mr, tri, cam, views)
    assert rc == -1
    eg, ed, em, er = mc.expected(tri, cam, views)
    assert np.array_equal(rects, er), (rects, er)
    assert np.array_equal(mask, em), np.argwhere(mask != em)[:5]
    assert np.array_equal(depth, ed), np.argwhere(depth != ed)[:5]
    assert np.array_equal(gray, eg), np.argwhere(gray != eg)[:5]
    covered = (em > 0).reshape(len(views), -1).sum(1)
    H, W = cam["height"], cam["width"]
    if name.endswith("outside"):
        assert covered.max() == 0 and not rects.any() and not gray.any() and not depth.any()
    else:
        assert covered.min() > 100    # the comparison is not about empty images (the smallest: cpu_binary at a third of the focal length)
    touches = {"left": er[0][0] == 0, "right": er[0][0] + er[0][2] == W, "top": er[0][1] == 0, "bottom": er[0][1] + er[0][3] == H}
    for side, hit in touches.items():
        if name == "chip_cut_" + side:
            assert hit and covered[0] > 3000 and er[0][2] * er[0][3] > 0
    if name == "chip_ties_degenerates":   # duplicates and degenerates change nothing: equal to the plain mesh
        pg, pd, pm, pr = mc.expected(ms.load_mesh("memoryChip2"), cam, views)
        assert np.array_equal(gray, pg) and np.array_equal(depth, pd) and np.array_equal(mask, pm) and np.array_equal(rects, pr)


def test_case_list_is_what_it_claims():
    names = [c[0] for c in CASES]
    assert len(CASES[0][3]) >= 60 and len(CASES[1][3]) >= 60 and len(set(names)) == len(names)
    tri = CASES[-1][1]
    assert len(tri) > len(ms.load_mesh("memoryChip2")) + 150


def test_vertex_behind_the_camera_invalidates_the_view(mr):
    chip, views = ms.load_mesh("memoryChip2"), ms.view_grid()
    cam = mc.camera(640, 480, mc.F)
    R_bad = mc.view_reaching_behind(chip, views, 0.02)
    with pytest.raises(ValueError):
        ms.render_view(chip, R_bad, 0.02, cam["fx"], cam["fy"], 640, 480)
    vs = [views[3], (R_bad, 0.02), views[4]]
    rc, gray, depth, mask, rects = host_render(mr, chip, cam, vs)
    assert rc == 1
    eg, ed, em, er = mc.expected(chip, cam, vs[:1])
    assert np.array_equal(gray[0], eg[0]) and np.array_equal(depth[0], ed[0]) and np.array_equal(mask[0], em[0]) and np.array_equal(rects[0], er[0])
    assert np.all(gray[1:] == 0x5a) and np.all(depth[1:] == 0x5a) and np.all(mask[1:] == 0x5a) and np.all(rects[1:] == -7)   # nothing written


# ---- argument checks of the C entry points (no device needed up to the point where LMX_ERR_NO_DEVICE is the answer) -----------------------

def _cam(width=640, height=480, f=mc.F, light=mc.LIGHT):
    return _lib.MeshCamera(width, height, f, f, width / 2.0, height / 2.0, (C.c_double * 3)(*light))


def _views(n=2, distance=0.5):
    v = (_lib.MeshView * n)()
    for i in range(n):
        v[i].R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        v[i].distance = distance
    return v


def _render(tri, n_tri, cam, views, n_views, outs=True):
    L = _lib.lib()
    H, W = 480, 640
    g = np.zeros((max(n_views, 1), H, W), np.uint8)
    r = np.zeros((max(n_views, 1), 4), np.int32)
    return L.lmx_mesh_render(0, tri.ctypes.data if tri is not None else None, n_tri, C.byref(cam) if cam is not None else None, views, n_views,
                             g.ctypes.data if outs else None, None, None, r.ctypes.data if outs else None)


def test_mesh_render_argument_checks():
    tri = np.ascontiguousarray(ms.load_mesh("memoryChip2"))
    L = _lib.lib()
    assert _render(None, 10, _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"null" in L.lmx_last_error()
    assert _render(tri, len(tri), None, _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(), None, 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, 0, _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"n_triangles" in L.lmx_last_error()
    assert _render(tri, -3, _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(), _views(), -1) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(width=0), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"camera" in L.lmx_last_error()
    assert _render(tri, len(tri), _cam(height=-4), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(f=float("nan")), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(f=0.0), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(light=(0.0, 0.0, 0.0)), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"light" in L.lmx_last_error()
    v = _views(3)
    v[1].R[4] = float("inf")
    assert _render(tri, len(tri), _cam(), v, 3) == _lib.LMX_ERR_INVALID_ARG and b"view 1" in L.lmx_last_error()
    v = _views(3)
    v[2].distance = float("nan")
    assert _render(tri, len(tri), _cam(), v, 3) == _lib.LMX_ERR_INVALID_ARG and b"view 2" in L.lmx_last_error()
    bad = tri.copy()
    bad[17, 1, 2] = float("nan")
    assert _render(bad, len(bad), _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"triangle 17" in L.lmx_last_error()
    # nothing to do: no device is touched
    assert _render(tri, len(tri), _cam(), _views(), 0) == _lib.LMX_OK
    if not has_gpu():
        assert _render(tri, len(tri), _cam(), _views(), 2) == _lib.LMX_ERR_NO_DEVICE


def test_bank_train_mesh_argument_checks():
    tri = np.ascontiguousarray(ms.load_mesh("memoryChip2"))
    L = _lib.lib()
    nb = NativeBank.from_bank(ms.empty_bank())
    cam, views = _cam(), _views()
    tp = tri.ctypes.data

    def call(bank=nb.h, t=tp, n=len(tri), c=cam, v=views, nv=2, cid=b"obj"):
        return L.lmx_bank_train_mesh(bank, 0, t, n, C.byref(c) if c is not None else None, v, nv, cid, None, None)

    assert call(bank=None) == _lib.LMX_ERR_INVALID_ARG and b"null" in L.lmx_last_error()
    assert call(t=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(c=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(v=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(cid=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(n=0) == _lib.LMX_ERR_INVALID_ARG
    assert call(nv=-2) == _lib.LMX_ERR_INVALID_ARG
    assert call(c=_cam(width=0)) == _lib.LMX_ERR_INVALID_ARG
    assert call(c=_cam(width=8, height=8)) == _lib.LMX_ERR_SHAPE          # lmx_bank_add_template's "source image too small"
    v = _views(2)
    v[0].R[0] = float("nan")
    assert call(v=v) == _lib.LMX_ERR_INVALID_ARG and b"view 0" in L.lmx_last_error()
    assert call(nv=0) == _lib.LMX_OK and L.lmx_bank_num_templates(nb.h, None) == 0
    side = C.POINTER(_lib.RendererParams)()
    assert L.lmx_bank_train_mesh(nb.h, 0, tp, len(tri), C.byref(cam), views, 0, b"obj", None, C.byref(side)) == _lib.LMX_OK
    assert side and side.contents.n_templates == 0 and side.contents.renderer_width == 640 and side.contents.renderer_focal_length_x == mc.F
    L.lmx_renderer_params_free(side)
    if not has_gpu():
        assert call() == _lib.LMX_ERR_NO_DEVICE
    assert L.lmx_bank_num_templates(nb.h, None) == 0
