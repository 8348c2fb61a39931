"""The two quantisers on the device on images where every pixel's label is its own (-m gpu).

tests/quantizer_images.py builds the frames -- depth whose normals change from pixel to pixel, read through random NORMAL_LUTs, colour
noise, gradients at the weak threshold, votes at the 5-of-9 rule, channels that tie with different orientations -- and
tests/test_quantizer_images_host.py shows on the CPU that they reach the median's and the colour compares' decision boundaries and that
the oracle equals the numpy restatement on each of them.  Here they go through every launch path of color_quantize_body and
depth_quantize_body (csrc/lmx_kernels.hip): the fused one-frame call with streamed rows, upload + enqueue, the plain kernels, batches
placed by frame, both colour tile heights, padded rows with garbage in the padding, gray contexts, the 64-bit depth form, both tables,
one, two and three pyramid levels, at sizes with ragged last tiles and interior (pipelined) depth tiles.  Every frame, level and modality:
labels, linear memories, the colour pyramid and the match list equal the oracle's.  The colour trainer's instantiation (squared
magnitudes written out) is compared through add_template.  Comparison: array_equal.
"""
import numpy as np
import pytest

import quantizer_images as qi
from linemod_pose_estimation_amd import Detector, NativeBank
from linemod_pose_estimation_amd.bank import DEFAULT_COLOR_GRADIENT, TemplateBank
from oracle import oracle as o

pytestmark = pytest.mark.gpu


def same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for k in ("x", "y", "similarity", "template_id", "class_index"):
        assert np.array_equal(a[k], b[k]), k


def _where(got, ref):
    bad = np.argwhere(got != ref)
    return len(bad), bad[:4].tolist()


@pytest.mark.parametrize("path", qi.PATHS, ids=[p[0] for p in qi.PATHS])
def test_device_equals_oracle_on_hostile_images(path, monkeypatch):
    name, W, H, mods, T, thr, frames, how, row_pad, env, gray, table = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)     # read when the context is created
    bank = qi.path_bank(path)
    given, seen = qi.path_sources(path)
    od = o.OracleDetector(bank)
    det = Detector(bank, W, H, max_batch=frames, max_candidates=1 << 16, gray=gray)
    if how == "match":
        assert frames == 1
        got = [det.match(given[0], qi.MATCH_THRESHOLD, cap=1 << 16)]
    elif how == "match_batch":
        got = det.match_batch(given, qi.MATCH_THRESHOLD, cap=1 << 16)
    else:
        det.upload(given)
        det.enqueue(frames, qi.MATCH_THRESHOLD)
        got = det.collect(frames, cap_total=frames << 16)
    n_cand = 0
    for f in range(frames):
        ref = od.match(seen[f], qi.MATCH_THRESHOLD)
        n_cand += od.last_candidates()
        for l in range(len(T)):
            for m, mod in enumerate(mods):
                q, rq = det.debug_quantized(f, l, m), od.quantized(l, m, (H >> l, W >> l))
                assert np.array_equal(q, rq), (name, "labels", f, l, mod) + _where(q, rq)
                lm, rlm = det.debug_linear_memory(f, l, m), od.linear_memory(l, m, (H >> l, W >> l))
                assert np.array_equal(lm, rlm), (name, "linear memory", f, l, mod)
        if "ColorGradient" in mods:
            cg = mods.index("ColorGradient")
            pyr = seen[f][cg]
            for l in range(1, len(T)):
                pyr = o.pyrdown(pyr)
                lv = det.debug_pyramid_bgr(f, l, cg)
                assert np.array_equal(lv, pyr[..., 0] if gray else pyr), (name, "pyramid", f, l)
        same(got[f], ref)
    assert det.stats()["candidates"] == n_cand
    det.close()


@pytest.mark.parametrize("kind", qi.TRAIN_KINDS)
def test_colour_trainer_on_hostile_views(kind):
    """lmx_bank_add_template on a 320 x 240 view of one colour family with a mask: the only user of the colour kernel's training form and of
    its squared magnitudes (extractTemplate ranks the candidates by them; "cross" is full of equal magnitudes).  Template id, box and every
    feature of both levels equal the oracle's addTemplate."""
    mdesc = [dict(DEFAULT_COLOR_GRADIENT, strong_threshold=qi.TRAIN_STRONG[kind])]
    od = o.OracleDetector(TemplateBank(T=[5, 8], modalities=mdesc))
    nb = NativeBank.create([5, 8], mdesc)
    bgr, mask = qi.training_view(kind)
    ref_tid, ref_bb = od.add_template([bgr], "obj", mask)
    got_tid, got_bb = nb.add_template([bgr], "obj", mask)
    assert ref_tid == 0 and (got_tid, got_bb) == (ref_tid, ref_bb)
    trained = nb.to_bank()
    assert trained.num_templates("obj") == 1
    for (w, h, lvl, f), (rw, rh, rl, rf) in zip(trained.get_templates("obj", 0), od.get_templates("obj", 0)):
        assert (w, h, lvl) == (rw, rh, rl) and np.array_equal(f, rf), (kind, lvl)
