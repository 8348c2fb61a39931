"""The depth-scored consumer chain without a device: dv::value (csrc/lmx_depth_verify.hpp, the one expression the scored kernel, the host
fallback and lmx_depth_value share) built with plain g++ from tests/cpp/depth_value_host.cpp against numpy's float64 and depth_values, the
same program under AddressSanitizer + UBSan as a child process, and the argument checks of the new entry points that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from linemod_pose_estimation_amd import DEPTH_DIFF_DTYPE, MATCH_DTYPE, DepthTemplates, _lib, depth_values
from linemod_pose_estimation_amd.detector import CLUSTER_DTYPE, RAW_MATCH_DTYPE

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "depth_value_host.cpp")
FLAGS = ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]

VALID = (0, 1, 2 ** 28)
SUMS = (0, 1, 2 ** 32, 2 ** 44 - 1)
NONE = (-np.inf, -1.5, 0.0)


def bits(v):
    return int(np.float64(v).view(np.uint64))


def expected_value(s, n, nv):
    """The issue's expression in numpy float64."""
    if n <= 0:
        return np.float64(nv)
    return -(np.float64(s) / (np.float64(n) * np.float64(1000.0)))


def table():
    return [(s, n, nv) for n in VALID for s in SUMS for nv in NONE]


def check_output(text):
    rows = [ln.split() for ln in text.strip().splitlines()]
    assert len(rows) == len(table()) == 36
    d = np.zeros(1, DEPTH_DIFF_DTYPE)
    for (s, n, nv), row in zip(table(), rows):
        assert (int(row[0]), int(row[1]), int(row[2], 16)) == (s, n, bits(nv)), row
        want = expected_value(s, n, nv)
        assert int(row[3], 16) == bits(want), (s, n, nv, row[3], "%016x" % bits(want))
        if nv == -np.inf:      # depth_values' choice of no_value
            d["sum_abs_mm"], d["n_valid"] = s, n
            assert int(row[3], 16) == bits(depth_values(d)[0]), (s, n)
    # what the table is for: the product n * 1000 beyond 2^32, a quotient that is not representable, -0.0 for a zero sum
    assert bits(expected_value(0, 1, 0.0)) == 1 << 63 and expected_value(2 ** 44 - 1, 2 ** 28, 0.0) != 0.0


def test_value_equals_numpy_float64_and_depth_values(tmp_path):
    exe = str(tmp_path / "depth_value_host")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    check_output(subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout)


def test_value_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "depth_value_host_san")
    subprocess.check_call(["g++"] + FLAGS + san + [SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    check_output(res.stdout)


def test_library_value_is_the_same_expression():
    L = _lib.lib()
    for s, n, nv in table():
        d = _lib.DepthDiff(s, n, n)
        assert bits(L.lmx_depth_value(C.byref(d), nv)) == bits(expected_value(s, n, nv)), (s, n, nv)
    assert L.lmx_depth_value(None, -1.5) == -1.5


def _image(a, channels=1, elem_size=2):
    return _lib.Image(a.ctypes.data, a.shape[0], a.shape[1], channels, elem_size, a.strides[0])


def test_argument_refusals_that_need_no_device():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16), np.zeros((0, 0), np.uint16)])   # two empty templates: no device touched
    d0, d1 = np.ones((12, 16), np.uint16), np.ones((12, 16), np.uint16)

    def upload(h=t.h, imgs=(d0, d1), images=None, nf=2):
        arr = images if images is not None else ((_lib.Image * len(imgs))(*[_image(a) for a in imgs]) if imgs is not None else None)
        return L.lmx_depth_templates_upload_scene(h, arr, nf)

    assert upload(h=None) == INV and b"null" in L.lmx_last_error()
    assert upload(imgs=None) == INV
    assert upload(nf=0) == INV and upload(nf=-2) == INV and b"n_frames" in L.lmx_last_error()
    bgr = np.ones((12, 16, 3), np.uint8)
    two = (_lib.Image * 2)(_image(d0), _lib.Image(bgr.ctypes.data, 12, 16, 3, 1, bgr.strides[0]))
    assert upload(images=two) == _lib.LMX_ERR_SHAPE and b"image 1" in L.lmx_last_error() and b"upload_scene" in L.lmx_last_error()
    assert upload(imgs=(d0, np.ones((12, 17), np.uint16))) == _lib.LMX_ERR_SHAPE and b"image 1 is 17 x 12" in L.lmx_last_error()
    assert upload(images=(_lib.Image * 2)(_image(d0), _lib.Image(None, 12, 16, 1, 2, 32))) == INV
    assert upload(images=(_lib.Image * 2)(_image(d0), _lib.Image(d1.ctypes.data, 12, 16, 1, 2, 30))) == _lib.LMX_ERR_SHAPE     # row stride below the row
    if not has_gpu():
        assert upload() == _lib.LMX_ERR_NO_DEVICE

    n = 4
    m, df = np.zeros(n, MATCH_DTYPE), np.zeros(n, DEPTH_DIFF_DTYPE)
    cl, mem = np.zeros(n, CLUSTER_DTYPE), np.zeros(n, np.int32)
    mo, co = (C.c_size_t * 3)(), (C.c_size_t * 3)()

    def collect(ctx=None, h=t.h, no_value=-np.inf):
        return L.lmx_ctx_collect_clusters_depth(ctx, 2, h, -1, no_value, m.ctypes.data, n, mo, df.ctypes.data, cl.ctypes.data, n, co, mem.ctypes.data, n)

    assert collect() == INV and b"null" in L.lmx_last_error()
    assert collect(h=None) == INV
    assert collect(no_value=float("nan")) == INV and b"not a number" in L.lmx_last_error()

    rec = np.zeros(3, RAW_MATCH_DTYPE)
    rec["order_key"] = np.arange(3)
    dists, rects = np.asarray([0.7, 0.7]), np.zeros((2, 4), np.int32)
    pp = _lib.ClusterParams(10, 0.5, 0.1, 2)
    M, D = np.zeros((2, 2048), MATCH_DTYPE), np.zeros((2, 2048), DEPTH_DIFF_DTYPE)
    CL, MEM, counts = np.zeros((2, 2048), CLUSTER_DTYPE), np.zeros((2, 2048), np.int32), np.zeros((2, 4), np.uint32)
    imgs = (_lib.Image * 2)(_image(d0), _image(d1))

    def hook(h=t.h, images=imgs, no_value=-np.inf, nf=2, diffs=D.ctypes.data, records=rec.ctypes.data):
        return L.lmx_debug_device_finalize_cluster_depth(0, records, len(rec), nf, h, images, -1, no_value, dists.ctypes.data, rects.ctypes.data, 2, C.byref(pp),
                                                         M.ctypes.data, diffs, CL.ctypes.data, MEM.ctypes.data, counts.ctypes.data)

    assert hook(h=None) == INV and hook(images=None) == INV and hook(diffs=None) == INV
    assert hook(no_value=float("nan")) == INV and b"not a number" in L.lmx_last_error()
    assert hook(nf=0) == INV and hook(nf=9) == INV and b"1..8" in L.lmx_last_error()
    if not has_gpu():
        assert hook() == _lib.LMX_ERR_NO_DEVICE
        assert hook(records=None) in (INV, _lib.LMX_ERR_NO_DEVICE)
    t.close()
