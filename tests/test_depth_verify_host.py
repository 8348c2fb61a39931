"""The depth check of matches without a device: the shared header (csrc/lmx_depth_verify.hpp, built with plain g++ from
tests/cpp/depth_verify_host.cpp) against the numpy restatement of tests/depth_verify_cases.py; the same file's main() under
AddressSanitizer + UBSan as a child process; the argument checks of every new entry point; lmx_cluster_matches_scored against
lmx_cluster_matches and on two constructed inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import depth_verify_cases as dvc
import mesh_cases as mc
from conftest import ROOT, has_gpu
from linemod_pose_estimation_amd import _lib, meshsynth as ms
from linemod_pose_estimation_amd import DEPTH_DIFF_DTYPE, MATCH_DTYPE, DepthTemplates, cluster_matches_scored, depth_values
from linemod_pose_estimation_amd.detector import CLUSTER_DTYPE, cluster_matches

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "depth_verify_host.cpp")
FLAGS = ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]


@pytest.fixture(scope="module")
def dv(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dvhost") / "libdvhost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.dv_host_pitch.argtypes = [C.c_int]
    lib.dv_host_diff.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]
    lib.dv_host_diff.restype = None
    return lib


def padded(lib, crop, fill):
    h, w = crop.shape
    pitch = lib.dv_host_pitch(w)
    assert pitch % 8 == 0 and w <= pitch < w + 8
    out = np.full((h, pitch), fill, np.uint16)
    out[:, :w] = crop
    return out


def host_diff(lib, pad, w, scene, x, y, vectors):
    out = np.zeros(3, np.int64)
    lib.dv_host_diff(pad.ctypes.data, w, pad.shape[0], pad.shape[1], scene.ctypes.data, scene.shape[1], scene.shape[0], scene.strides[0] // 2, int(x), int(y),
                     vectors, out.ctypes.data)
    return out


def test_header_equals_the_numpy_restatement(dv):
    crops, scene, matches, expected = dvc.constructed()
    zero = [padded(dv, c, 0) for c in crops]
    junk = [padded(dv, c, 0xbeef) for c in crops]        # the pixel walk never reads the padding
    wide = np.zeros((dvc.SCENE_H, dvc.SCENE_W + 5), np.uint16)   # the same scene as a strided view
    wide[:, :dvc.SCENE_W] = scene
    wide[:, dvc.SCENE_W:] = 777
    for (x, y, k), want in zip(matches, expected):
        w = crops[k].shape[1]
        assert np.array_equal(host_diff(dv, junk[k], w, scene, x, y, 0), want), (x, y, crops[k].shape)
        assert np.array_equal(host_diff(dv, zero[k], w, scene, x, y, 1), want), (x, y, crops[k].shape)
        assert np.array_equal(host_diff(dv, zero[k], w, wide[:, :dvc.SCENE_W], x, y, 1), want), (x, y, crops[k].shape)


def test_header_sum_does_not_wrap_at_2_to_32(dv):
    crop = np.full((256, 257), 65535, np.uint16)
    scene = np.ones((300, 300), np.uint16)
    assert dvc.np_diff(crop, scene, 20, 30) == (4311612928, 65792, 65792) and 65534 * 65792 == 4311612928
    for vectors in (0, 1):
        assert host_diff(dv, padded(dv, crop, 0), 257, scene, 20, 30, vectors).tolist() == [4311612928, 65792, 65792]


def test_border_cases_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "depth_verify_host")
    subprocess.check_call(["g++"] + FLAGS + san + [SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "depth_verify_host ok" in res.stdout


# ---- argument checks (no device needed up to the point where LMX_ERR_NO_DEVICE is the answer) ------------------------------------------

def _cam(width=320, height=240, f=mc.F / 2):
    return _lib.MeshCamera(width, height, f, f, width / 2.0, height / 2.0, (C.c_double * 3)(*mc.LIGHT))


def _views(n=2, distance=0.5):
    v = (_lib.MeshView * n)()
    for i in range(n):
        v[i].R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        v[i].distance = distance
    return v


def _image(a, channels=1, elem_size=2):
    return _lib.Image(a.ctypes.data, a.shape[0], a.shape[1], channels, elem_size, a.strides[0])


def test_depth_templates_constructor_argument_checks():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    tri = np.ascontiguousarray(ms.load_mesh("memoryChip2"))
    h = C.c_void_p()

    def mesh(t=tri.ctypes.data, n=len(tri), c=_cam(), v=_views(), nv=2, out=C.byref(h)):
        return L.lmx_depth_templates_from_mesh(0, t, n, C.byref(c) if c is not None else None, v, nv, out)

    assert mesh(out=None) == INV and b"null" in L.lmx_last_error()
    assert mesh(t=None) == INV and mesh(c=None) == INV and mesh(v=None) == INV
    assert mesh(n=0) == INV and mesh(n=-3) == INV and mesh(nv=-1) == INV and b"n_views" in L.lmx_last_error()
    assert mesh(c=_cam(width=0)) == INV
    bad = _views(3)
    bad[1].R[4] = float("nan")
    assert mesh(v=bad, nv=3) == INV and b"view 1" in L.lmx_last_error()
    behind = _views(3)
    behind[2].distance = 0.0          # the mesh around the camera: a vertex at Z <= 0.01, found on the host before any device work
    assert mesh(v=behind, nv=3) == INV and b"view 2 " in L.lmx_last_error()
    assert h.value is None
    assert mesh(nv=0) == _lib.LMX_OK and h.value and L.lmx_depth_templates_count(h) == 0 and L.lmx_depth_templates_device_bytes(h) == 0
    L.lmx_depth_templates_free(h)
    L.lmx_depth_templates_free(None)
    if not has_gpu():
        assert mesh() == _lib.LMX_ERR_NO_DEVICE

    crop = np.ones((3, 5), np.uint16)
    ptrs = (C.c_void_p * 2)(crop.ctypes.data, crop.ctypes.data)

    def crops(p=ptrs, sizes=(5, 3, 5, 3), n=2, out=C.byref(h)):
        return L.lmx_depth_templates_from_crops(0, p, (C.c_int32 * len(sizes))(*sizes) if sizes is not None else None, n, out)

    h.value = None
    assert crops(out=None) == INV and crops(p=None) == INV and crops(sizes=None) == INV and b"null" in L.lmx_last_error()
    assert crops(n=-1) == INV
    assert crops(sizes=(5, 3, -1, 3)) == INV and b"crop 1" in L.lmx_last_error()
    assert crops(sizes=(5, -2, 5, 3)) == INV and b"crop 0" in L.lmx_last_error()
    assert crops(sizes=(16385, 1, 5, 3)) == INV and crops(sizes=(5, 3, 1, 16385)) == INV and b"crop 1" in L.lmx_last_error()
    assert crops(p=(C.c_void_p * 2)(crop.ctypes.data, None)) == INV and b"crop 1 is null" in L.lmx_last_error()
    assert h.value is None
    # nothing that needs a device: no crops, or empty ones only (their pointers are not read)
    assert crops(p=None, sizes=None, n=0) == _lib.LMX_OK and L.lmx_depth_templates_count(h) == 0
    L.lmx_depth_templates_free(h)
    h.value = None
    assert crops(p=(C.c_void_p * 2)(None, None), sizes=(0, 0, 0, 7)) == _lib.LMX_OK and L.lmx_depth_templates_count(h) == 2
    r = (C.c_int32 * 4)(9, 9, 9, 9)
    assert L.lmx_depth_templates_rect(h, 1, r) == _lib.LMX_OK and list(r) == [0, 0, 0, 0]
    assert L.lmx_depth_templates_device_bytes(h) == 2 * 24
    L.lmx_depth_templates_free(h)
    if not has_gpu():
        assert crops() == _lib.LMX_ERR_NO_DEVICE


def test_depth_templates_accessor_and_diff_argument_checks():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16), np.zeros((0, 0), np.uint16)])   # two empty templates: no device touched
    assert len(t) == 2 and t.crop(1).shape == (0, 0) and t.rect(0) == (0, 0, 0, 0)
    r = (C.c_int32 * 4)()
    assert L.lmx_depth_templates_count(None) == 0 and L.lmx_depth_templates_device_bytes(None) == 0
    assert L.lmx_depth_templates_rect(None, 0, r) == INV and L.lmx_depth_templates_rect(t.h, 0, None) == INV
    assert L.lmx_depth_templates_rect(t.h, 2, r) == INV and b"id 2" in L.lmx_last_error()
    assert L.lmx_depth_templates_rect(t.h, -1, r) == INV
    buf = np.zeros(4, np.uint16)
    assert L.lmx_depth_templates_get(None, 0, buf.ctypes.data) == INV
    assert L.lmx_depth_templates_get(t.h, 2, buf.ctypes.data) == INV and b"id 2" in L.lmx_last_error()
    assert L.lmx_depth_templates_get(t.h, -1, buf.ctypes.data) == INV

    d0, d1 = np.ones((12, 16), np.uint16), np.ones((12, 16), np.uint16)
    m = np.zeros(3, MATCH_DTYPE)
    out = np.full(3, 7, DEPTH_DIFF_DTYPE)

    def diff(h=t.h, imgs=(d0, d1), images=None, nf=2, matches=m, offsets=(0, 1, 3), cls=-1, o=out):
        arr = images if images is not None else ((_lib.Image * len(imgs))(*[_image(a) for a in imgs]) if imgs is not None else None)
        offs = (C.c_size_t * len(offsets))(*offsets) if offsets is not None else None
        return L.lmx_depth_diff_matches(h, arr, nf, matches.ctypes.data if matches is not None else None, offs, cls, o.ctypes.data if o is not None else None)

    assert diff(h=None) == INV and b"null" in L.lmx_last_error()
    assert diff(imgs=None) == INV and diff(offsets=None) == INV and diff(matches=None) == INV and diff(o=None) == INV
    assert diff(nf=-1) == INV and b"n_frames" in L.lmx_last_error()
    assert diff(offsets=(1, 1, 3)) == INV and diff(offsets=(0, 2, 1)) == INV and b"offsets" in L.lmx_last_error()
    bgr = np.ones((12, 16, 3), np.uint8)
    two = (_lib.Image * 2)(_image(d0), _lib.Image(bgr.ctypes.data, 12, 16, 3, 1, bgr.strides[0]))
    assert diff(images=two) == _lib.LMX_ERR_SHAPE and b"image 1" in L.lmx_last_error() and b"one channel of 2 bytes" in L.lmx_last_error()
    assert diff(images=(_lib.Image * 2)(_image(d0), _image(d1, elem_size=4))) == _lib.LMX_ERR_SHAPE
    assert diff(images=(_lib.Image * 2)(_image(d0), _image(d1, channels=2))) == _lib.LMX_ERR_SHAPE
    assert diff(imgs=(d0, np.ones((12, 17), np.uint16))) == _lib.LMX_ERR_SHAPE and b"image 1 is 17 x 12" in L.lmx_last_error()
    assert diff(imgs=(d0, np.ones((11, 16), np.uint16))) == _lib.LMX_ERR_SHAPE
    assert diff(images=(_lib.Image * 2)(_image(d0), _lib.Image(None, 12, 16, 1, 2, 32))) == INV
    bad = m.copy()
    bad["template_id"][2] = 2
    assert diff(matches=bad) == INV and b"match 2" in L.lmx_last_error() and b"template_id 2" in L.lmx_last_error()
    bad["template_id"][2] = -1
    assert diff(matches=bad) == INV and b"match 2" in L.lmx_last_error()
    bad["class_index"][2] = 4                 # another class's match: its template id is not this object's to judge
    bad["class_index"][:2] = 1
    assert diff(matches=bad, cls=0) == _lib.LMX_OK and not out.view(np.uint8).any()       # nothing selected: zeros, no device
    # nothing to do: no device is touched
    out[:] = 7
    assert diff(nf=0, imgs=None, offsets=None, matches=None, o=None) == _lib.LMX_OK
    assert diff(offsets=(0, 0, 0), matches=None, o=None) == _lib.LMX_OK
    if not has_gpu():
        assert diff() == _lib.LMX_ERR_NO_DEVICE      # valid matches of (empty) templates need the device
    t.close()
    t.close()


# ---- lmx_cluster_matches_scored ------------------------------------------------------------------------------------------------------------

def test_scored_with_similarities_equals_cluster_matches_on_every_case():
    n_frames = n_clusters = 0
    for case in cc.cases():
        for ref in cc.reference(case):
            m = np.ascontiguousarray(ref.matches).astype(MATCH_DTYPE)
            args = (case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)
            if ref.clusters is None:     # a template id outside the side-car: both refuse it
                for call in (lambda: cluster_matches(m, *args), lambda: cluster_matches_scored(m, m["similarity"].astype(np.float64), *args)):
                    with pytest.raises(_lib.LmxError) as e:
                        call()
                    assert e.value.status == _lib.LMX_ERR_INVALID_ARG
                continue
            c0, mem0 = cluster_matches(m, *args)
            c1, mem1 = cluster_matches_scored(m, m["similarity"].astype(np.float64), *args)
            assert len(c0) == len(c1) and np.array_equal(mem0, mem1), case.name
            for k in cc.CLUSTER_FIELDS:       # field by field (the records have padding); the scores bit for bit
                assert c0[k].tobytes() == c1[k].tobytes(), (case.name, k)
                assert np.array_equal(c0[k], ref.clusters[k]), (case.name, k)
            n_frames += 1
            n_clusters += len(c0)
    assert n_frames > 20 and n_clusters > 100


def _bins_case(positions, per_cluster, rect_side):
    """One cluster per position: `per_cluster` matches inside one voting bin of 10 px, template 0 with a rect_side^2 rect."""
    rows = [(x + k, y + k, 0) for (x, y) in positions for k in range(per_cluster)]
    m = dvc.match_records(MATCH_DTYPE, rows)
    return m, np.asarray([0.72]), np.asarray([[0, 0, rect_side, rect_side]], np.int32)


def test_scored_orders_clusters_by_the_values_not_the_similarities():
    pos = [(0, 0), (100, 0), (200, 0), (0, 100), (100, 100)]
    m, dists, rects = _bins_case(pos, 3, 20)       # 100 px apart, 20 px rects: nothing overlaps
    sims = [95.0, 90.0, 85.0, 80.0, 75.0]
    means = [-0.30, -0.01, -0.20, -0.002, -0.10]   # minus metres: well separated, in another order than the similarities
    values = np.zeros(len(m))
    for c in range(5):
        m["similarity"][3 * c:3 * c + 3] = sims[c]
        values[3 * c:3 * c + 3] = np.asarray([0.5, 1.0, 1.5]) * means[c]
    args = (dists, rects, 10, 0.5, 0.1, 2)
    by_sim, _ = cluster_matches(m, *args)
    by_val, mem = cluster_matches_scored(m, values, *args)
    assert [tuple(c["rect"][:2]) for c in by_sim] == [(x + 1, y + 1) for x, y in pos]
    want = [pos[c] for c in np.argsort(means)[::-1]]
    assert [tuple(c["rect"][:2]) for c in by_val] == [(x + 1, y + 1) for x, y in want] and want != pos
    for c in by_val:
        mi = mem[c["member_begin"]:c["member_begin"] + c["member_count"]]
        assert c["member_count"] == 3 and c["score"] == (values[mi[0]] + values[mi[1]] + values[mi[2]]) / 3     # the mean in voting order
    # -inf (depth_values' choice for n_valid == 0) sends a cluster to the end; a NaN mean is refused
    v2 = values.copy()
    v2[3] = -np.inf
    last, _ = cluster_matches_scored(m, v2, *args)
    assert tuple(last[-1]["rect"][:2]) == (101, 1) and last[-1]["score"] == -np.inf and len(last) == 5
    v2[4] = np.inf
    with pytest.raises(_lib.LmxError) as e:
        cluster_matches_scored(m, v2, *args)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "not a number" in str(e.value)
    with pytest.raises(ValueError):
        cluster_matches_scored(m, values[:-1], *args)
    n = C.c_size_t()
    pp = _lib.ClusterParams(10, 0.5, 0.1, 2)
    cl = np.zeros(8, CLUSTER_DTYPE)
    assert _lib.lib().lmx_cluster_matches_scored(m.ctypes.data, len(m), None, dists.ctypes.data, rects.ctypes.data, 1, C.byref(pp), cl.ctypes.data, 8,
                                                 C.byref(n), mem.ctypes.data, len(mem)) == _lib.LMX_ERR_INVALID_ARG


def test_scored_values_reverse_which_overlapping_cluster_survives():
    m, dists, rects = _bins_case([(0, 0), (10, 0)], 3, 30)      # 30 px rects 10 px apart: IoU 0.5 > 0.4
    m["similarity"][:3], m["similarity"][3:] = 90.0, 80.0
    values = np.asarray([-0.2, -0.2, -0.2, -0.004, -0.004, -0.004])
    args = (dists, rects, 10, 0.5, 0.1, 2)
    by_sim, _ = cluster_matches(m, *args)
    by_val, mem = cluster_matches_scored(m, values, *args)
    assert len(by_sim) == 1 and tuple(by_sim[0]["rect"]) == (1, 1, 30, 30) and by_sim[0]["score"] == 90.0
    assert len(by_val) == 1 and tuple(by_val[0]["rect"]) == (11, 1, 30, 30) and by_val[0]["score"] == np.mean(values[3:])
    assert sorted(mem[:3]) == [3, 4, 5]


def test_depth_values():
    d = np.zeros(4, DEPTH_DIFF_DTYPE)
    d["sum_abs_mm"], d["n_valid"], d["n_template"] = [0, 7000, 4311612928, 0], [10, 7, 65792, 0], [10, 9, 65792, 5]
    v = depth_values(d)
    assert v[0] == 0.0 and v[1] == -1.0 and v[2] == -(4311612928 / (65792 * 1000.0)) and v[3] == -np.inf
