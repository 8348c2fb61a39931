"""The 16-byte load phase of the spread kernels (spread_linearize_t_body in csrc/lmx_kernels.hip: four dwords of a label row per item where
W % 16 == 0 and the label image is 16-byte aligned, the dword loop otherwise) against the CPU oracle, byte for byte through the debug reads:
the level-0 spread image of both modalities, the coarsest level's memories and the final matches.

Shapes and what they reach (level 0 is banded in all of them, Wc % 16 == 0 and Wc >= 32, hence W % 16 == 0):
  T = {5, 8}  160 x 80    2 bands; level 1 is 80 x 40: 16-byte loads with aligned 16-byte LDS writes, byte-wide memories (Wc = 10)
              240 x 160   3 bands; level 1 is 120 x 80: W % 16 != 0 and Wc = 15, the generic kernel
              320 x 240   4 bands, Hc = 48; level 1 is 160 x 120: 16-byte loads, byte-wide memories (Wc = 20)
              640 x 480   the headline's shape, one frame: level 1 is nibble-packed, both levels in one k_small_spread<5, 8> launch
  T = {4, 8}  128 x 64    2 bands; level 1 is 64 x 32, nibble-packed: k_small_spread<4, 8>
              256 x 192   4 bands; level 1 is 128 x 96, nibble-packed: k_small_spread<4, 8>
One and two frames take the small-batch chain (k_small_spread where the level pair has a fused kernel), three the per-level launches with
the plain grid, nine the XCD-aware placement (n_frames_x > 0) with seven empty slots in its second group of eight."""
import numpy as np
import pytest

from linemod_pose_estimation_amd import Detector, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

THR = 58.0
MODS = ("ColorGradient", "DepthNormal")


def same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for k in ("x", "y", "similarity", "template_id", "class_index"):
        assert np.array_equal(a[k], b[k]), k


def check_stages(det, od, W, H, L, M, frame=0):
    """Label images and linear memories (finer levels: the spread image, un-banded by the debug read) of every level and modality."""
    for l in range(L):
        for m in range(M):
            assert np.array_equal(det.debug_quantized(frame, l, m), od.quantized(l, m, (H >> l, W >> l))), ("quant", l, m)
            assert np.array_equal(det.debug_linear_memory(frame, l, m), od.linear_memory(l, m, (H >> l, W >> l))), ("lm", l, m)


def _bank(W, H, T, seed):
    return synth.make_bank(24, modalities=MODS, T=T, seed=seed, size_range=(16.0, min(W, H) * 0.45))


def _scene(bank, W, H, seed):
    """synth.make_scene places its instances at least 40 px from every border: the small shapes are the middle of a larger scene."""
    if min(W, H) > 100:
        return synth.make_scene(bank, W, H, seed=seed, n_instances=4)[0]
    big = synth.make_scene(bank, W + 120, H + 120, seed=seed, n_instances=8)[0]
    return [np.ascontiguousarray(a[60:60 + H, 60:60 + W]) for a in big]


def _run_batch(bank, W, H, frames):
    od = o.OracleDetector(bank)
    det = Detector(bank, W, H, max_batch=len(frames), max_candidates=1 << 18)
    det.upload(frames)
    det.enqueue(len(frames), THR)
    got = det.collect(len(frames))
    n_matches = n_candidates = 0
    for f in sorted({0, 7, len(frames) - 1} & set(range(len(frames)))):
        ref = od.match(frames[f], THR)       # the oracle keeps this frame's stages for check_stages
        check_stages(det, od, W, H, len(bank.T), 2, frame=f)
        same(got[f], ref)
        n_matches += len(ref)
        n_candidates += od.last_candidates()
    det.close()
    # the templates hardly fit the smallest shapes: there the refinement still reads the spread image for every candidate, but none passes
    assert n_candidates > 100 and (n_matches > 0 or min(W, H) <= 100), (n_candidates, n_matches)


@pytest.mark.parametrize("W,H,T,n_frames", [
    (160, 80, (5, 8), 1), (240, 160, (5, 8), 2), (320, 240, (5, 8), 1), (640, 480, (5, 8), 1),
    (128, 64, (4, 8), 2), (256, 192, (4, 8), 1),
    (240, 160, (5, 8), 3), (256, 192, (4, 8), 3),
])
def test_spread_images_memories_and_matches_equal_the_oracle(W, H, T, n_frames):
    bank = _bank(W, H, T, seed=1200 + W)
    frames = [_scene(bank, W, H, 1300 + W + f) for f in range(n_frames)]
    _run_batch(bank, W, H, frames)


def test_nine_frames_leave_the_last_xcd_group_partly_empty():
    W, H = 160, 80
    bank = _bank(W, H, (5, 8), seed=1209)
    frames = [_scene(bank, W, H, 1400 + f) for f in range(9)]
    _run_batch(bank, W, H, frames)


def test_masked_labels_reach_the_spread():
    """k_apply_mask clears labels before the spread reads them: a blocky mask on each modality, one frame."""
    W, H = 320, 240
    bank = _bank(W, H, (5, 8), seed=1210)
    src = _scene(bank, W, H, 1500)
    rng = np.random.default_rng(12)
    masks = [np.ascontiguousarray(np.kron((rng.uniform(0, 1, (H // 16, W // 16)) < p).astype(np.uint8) * 255, np.ones((16, 16), np.uint8))) for p in (0.7, 0.8)]
    od = o.OracleDetector(bank)
    ref = od.match(src, THR, masks=masks)
    det = Detector(bank, W, H, max_candidates=1 << 18)
    got = det.match_masked(src, masks, THR)
    check_stages(det, od, W, H, 2, 2)
    same(got, ref)
    assert 0 < len(ref) < len(od.match(src, THR))
    det.close()
