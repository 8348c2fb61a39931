"""The colour quantiser's one-plane path (color_quantize_tile<TH, TRAIN, 1>, the gray context LMX_CTX_GRAY) on the CPU (tests/cpp/cq_host_gray.cpp:
linemod_pose_estimation_amd/csrc/lmx_color_quantize.hpp compiled with LMX_CQ_HOST) against the oracle run on the gray image copied into B, G and R:
labels, the one-byte pyrDown (= channel 0 of the BGR pyrDown) and the trainer's squared magnitudes, bit for bit -- image borders, sizes that are no
multiple of the tile, odd sizes, both tile heights.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as o

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")


@pytest.fixture(scope="module")
def cq(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cqhostgray") / "libcqhostgray.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "cq_host_gray.cpp")])
    lib = C.CDLL(so)
    lib.cq_host_gray_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int]
    return lib


def run(lib, gray, th, weak=10.0, pyr=True, mag=False):
    H, W = gray.shape
    dst = np.full((H, W), 0x5a, np.uint8)
    pd = np.full((H // 2, W // 2), 0x5a, np.uint8) if pyr else None
    mg = np.full((H, W), -1.0, np.float32) if mag else None
    rc = lib.cq_host_gray_run(gray.ctypes.data, dst.ctypes.data, pd.ctypes.data if pyr else None, mg.ctypes.data if mag else None, H, W, C.c_float(weak), th)
    assert rc == 0
    return dst, pd, mg


def gray_image(rng, H, W, kind):
    if kind == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "smooth":   # gradients strong enough to pass the weak threshold, low-pass so that votes reach 5 of 9
        a = np.kron(rng.uniform(0, 255, (H // 8 + 2, W // 8 + 2)), np.ones((8, 8)))[:H, :W]
        return np.ascontiguousarray(np.clip(a + rng.normal(0, 3, a.shape), 0, 255).astype(np.uint8))
    if kind == "extreme":  # saturating blocks: Sobel outputs reach +-1020
        a = (rng.integers(0, 2, (H // 4 + 1, W // 4 + 1)) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.kron(a, np.ones((4, 4), np.uint8))[:H, :W])
    if kind == "ramp":     # one orientation everywhere, the borders carry the only structure
        y, x = np.mgrid[0:H, 0:W]
        return np.ascontiguousarray(((x * 7 + y * 3) % 256).astype(np.uint8))
    raise ValueError(kind)


def bgr_of(gray):
    return np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=2))


@pytest.mark.parametrize("H,W", [(96, 128), (64, 64), (37, 70), (33, 131), (16, 8), (5, 4), (4, 5), (130, 66), (67, 257), (240, 320), (75, 139)])
@pytest.mark.parametrize("th", [16, 32])
def test_gray_labels_pyrdown_and_magnitudes_equal_the_oracle_on_replicated_bgr(cq, H, W, th):
    rng = np.random.default_rng(H * 1000 + W + th + 7)
    for kind in ("smooth", "noise", "extreme", "ramp"):
        g = gray_image(rng, H, W, kind)
        bgr = bgr_of(g)
        ref_q, ref_mag, _ = o.quantized_orientations(bgr, 10.0)
        dst, pd, mg = run(cq, g, th, mag=True)
        assert np.array_equal(dst, ref_q), (kind, np.argwhere(dst != ref_q)[:5])
        ref_pd = o.pyrdown(bgr)
        assert np.array_equal(pd, ref_pd[..., 0]), (kind, np.argwhere(pd != ref_pd[..., 0])[:5])
        assert np.array_equal(mg, ref_mag), (kind, np.argwhere(mg != ref_mag)[:5])
        if kind == "smooth" and H * W > 4000:
            assert (ref_q != 0).mean() > 0.05           # the comparison is not about empty images
    # the inference instantiation (no magnitudes), no pyramid output (the coarsest level), another weak threshold
    g = gray_image(rng, H, W, "smooth")
    dst, pd, _ = run(cq, g, th, weak=25.0)
    assert np.array_equal(dst, o.quantized_orientations(bgr_of(g), 25.0)[0])
    assert np.array_equal(pd, o.pyrdown(bgr_of(g))[..., 0])
    dst, _, _ = run(cq, g, th, weak=25.0, pyr=False)
    assert np.array_equal(dst, o.quantized_orientations(bgr_of(g), 25.0)[0])


def test_gray_pyramid_levels_chain(cq):
    """Level l + 1 is quantised from the one-byte pyrDown of level l: three levels equal the oracle's BGR chain, channel 0."""
    rng = np.random.default_rng(5)
    g = gray_image(rng, 240, 320, "smooth")
    bgr = bgr_of(g)
    for _ in range(3):
        dst, pd, _ = run(cq, g, 16)
        assert np.array_equal(dst, o.quantized_orientations(bgr, 10.0)[0])
        bgr = o.pyrdown(bgr)
        assert np.array_equal(pd, bgr[..., 0])
        g = np.ascontiguousarray(pd)


def test_gray_lds_budget(cq):
    """The one-plane tile needs region 2 for its label / flag planes (larger than its one-plane blur rows): about 15 KB at TH = 32."""
    for th, bound in ((32, 15 * 1024), (16, 9 * 1024)):
        assert cq.cq_host_gray_lds_bytes(th) <= bound
