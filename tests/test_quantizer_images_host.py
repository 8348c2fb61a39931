"""The hostile quantiser images of tests/quantizer_images.py on the CPU: for every frame tests/test_gpu_quantizer_images.py sends through
the device, the oracle equals the numpy restatement (labels before the median, after it, colour labels, every pyramid level) -- the
known-answer tests of test_oracle_kat.py use tame inputs, so on these images that is not a given -- and the frames reach the kernels'
decision boundaries: the coverage conditions below are conditions on the INPUTS (a recipe that misses one is changed, never the
condition).  The colour kernel's CPU emulation runs on the two new colour families, and planted faults (a median of the wrong rank,
labels written to the wrong place) are counted on a synthetic scene and on a hostile image.  DESIGN.md records the printed counts.
"""
import numpy as np
import pytest

import np_restatement as R
import quantizer_images as qi
from linemod_pose_estimation_amd import synth
from oracle import oracle as o
from test_color_kernel_host import SIZES, cq, run   # noqa: F401  (cq: the module-scoped fixture that builds the emulation)

IDS = [p[0] for p in qi.PATHS]


@pytest.mark.parametrize("path", qi.PATHS, ids=IDS)
def test_oracle_equals_restatement_on_every_device_frame(path):
    name, W, H, mods, T, thr = path[:6]
    bank = qi.path_bank(path)
    od = o.OracleDetector(bank)
    given, seen = qi.path_sources(path)
    n_match = n_cand = 0
    for f, (depth, bgr, kind) in enumerate(qi.path_frames(path)):
        for a, b in zip(given[f], seen[f]):       # what the context is handed holds the oracle's pixels (a gray plane: channel 0); padded rows are views
            assert np.array_equal(a, b if a.ndim == b.ndim else b[..., 0]) and a.flags["C_CONTIGUOUS"] == (path[8] == 0)
            assert path[8] == 0 or (a.base[:, W:] != 0).all()     # non-zero garbage behind every row
        if depth is not None:
            q, pre = o.quantized_normals(depth, qi.DIST, thr, bank.normal_lut)
            rq, rpre = R.quantized_normals(depth, qi.DIST, thr, bank.normal_lut)
            assert np.array_equal(pre, rpre), (name, f, "before the median")
            assert np.array_equal(q, rq), (name, f, "after the median")
            assert np.array_equal(q, qi.median_of_counts(qi.window_counts(pre))), (name, f, "the counter's median")
        if bgr is not None:
            src = seen[f][mods.index("ColorGradient")]
            assert np.array_equal(o.quantized_orientations(src, 10.0)[0], R.quantized_orientations(src, 10.0)[0]), (name, f, kind)
        n_match += len(od.match(seen[f], qi.MATCH_THRESHOLD))
        n_cand += od.last_candidates()
        labels = R.quantize_pyramid(bank, seen[f])
        for l in range(len(T)):
            for m in range(len(mods)):
                assert np.array_equal(od.quantized(l, m, (H >> l, W >> l)), labels[l][m]), (name, f, l, m)
    print("%s: %d candidates, %d matches at threshold %g" % (name, n_cand, n_match, qi.MATCH_THRESHOLD))
    assert n_cand < (1 << 16) * path[6]


def _first_frame(size, table):
    """frame 0 of the first device path of that size and table -> (label map before the median, path name)"""
    for path in qi.PATHS:
        if (path[1], path[2]) == size and "DepthNormal" in path[3] and path[11] == table:
            depth = qi.path_frames(path)[0][0]
            return o.quantized_normals(depth, qi.DIST, path[5], qi.normal_table(table))[1], path[0]
    raise KeyError((size, table))


@pytest.mark.parametrize("size", sorted({(p[1], p[2]) for p in qi.PATHS}))
def test_depth_images_reach_the_medians_boundaries(size):
    """Per size, summed over one image of either table: every median value 0..64 has >= 40 windows with #(<= v) == 13 and every value 1..128
    >= 10 windows with #(< v) == 12 (the two sides of the counting median's `+ 19` carry), >= 500 windows hold all nine values, and under
    the uniform table at most 20 % of the horizontally adjacent labels inside the frame are equal."""
    le13, lt12, nine = np.zeros(9, np.int64), np.zeros(9, np.int64), 0
    for table in ("uniform", "high"):
        pre, name = _first_frame(size, table)
        c = qi.depth_coverage(pre)
        le13 += c["le13"]; lt12 += c["lt12"]; nine += int(c["distinct"][9])
        print("%dx%d %s (%s): distinct values per window %s, equal neighbours %.1f %%" % (size + (table, name, c["distinct"][1:].tolist(), 100 * c["equal_neighbours"])))
        if table == "uniform":
            assert c["equal_neighbours"] <= 0.20
    print("%dx%d #(<= v) == 13 per median value 0..64:  %s" % (size + (le13[:8].tolist(),)))
    print("%dx%d #(< v) == 12 per median value 1..128: %s; nine-value windows: %d" % (size + (lt12[1:].tolist(), nine)))
    assert le13[:8].min() >= 40 and le13[8] == 0
    assert lt12[1:].min() >= 10 and lt12[0] == 0
    assert nine >= 500


def test_colour_images_reach_the_threshold_the_vote_rule_and_the_channel_tie():
    """Summed over the colour frames the device tests use, per family: faint -> >= 10 pixels whose strongest squared magnitude is exactly
    weak_threshold ** 2, >= 10 within 4 below, >= 10 within 4 above; noise + smooth -> >= 100 strong pixels whose best vote is 4 and >= 100
    whose best vote is 5; cross -> >= 100 pixels where two channels tie above the threshold with different labels of their own."""
    total = {k: dict(at=0, below=0, above=0, vote4=0, vote5=0, tied=0, frames=0) for k in qi.COLOR_KINDS}
    for path in qi.PATHS:
        if "ColorGradient" not in path[3]:
            continue
        _, seen = qi.path_sources(path)
        for f, (_, _, kind) in enumerate(qi.path_frames(path)):
            c = qi.color_coverage(seen[f][path[3].index("ColorGradient")])
            for k, v in c.items():
                total[kind][k] += v
            total[kind]["frames"] += 1
    for kind in qi.COLOR_KINDS:
        print("colour %-8s %s" % (kind, total[kind]))
    assert min(total["faint"][k] for k in ("at", "below", "above")) >= 10
    assert total["noise"]["vote4"] + total["smooth"]["vote4"] >= 100 and total["noise"]["vote5"] + total["smooth"]["vote5"] >= 100
    assert total["cross"]["tied"] >= 100
    one = qi.color_coverage(qi.color_image(np.random.default_rng(3), 72, 136, "cross"))   # one BGR image suffices for the tie
    assert one["tied"] >= 100
    assert qi.color_coverage(qi.color_image(np.random.default_rng(3), 72, 136, "extreme"))["tied"] == 0   # replicated planes cannot show precedence


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("th", [16, 32])
def test_colour_emulation_on_faint_and_cross(cq, H, W, th):
    """the colour kernel's CPU emulation (test_color_kernel_host.py) on the two new families: labels, pyrDown and squared magnitudes"""
    rng = np.random.default_rng(H * 1000 + W + th + 7)
    for kind in ("faint", "cross"):
        bgr = qi.color_image(rng, H, W, kind)
        ref_q, ref_mag, _ = o.quantized_orientations(bgr, 10.0)
        dst, pd, mg = run(cq, bgr, th, mag=True)
        assert np.array_equal(dst, ref_q), (kind, np.argwhere(dst != ref_q)[:5])
        assert np.array_equal(pd, o.pyrdown(bgr)), kind
        assert np.array_equal(mg, ref_mag), kind
        g, rep = qi.gray_plane(bgr)
        assert np.array_equal(run(cq, rep, th)[0], o.quantized_orientations(rep, 10.0)[0]), kind


def test_training_views_are_accepted_by_the_oracle():
    """the views of the device trainer test give a template each (a rejected view would compare -1 with -1)"""
    from linemod_pose_estimation_amd.bank import DEFAULT_COLOR_GRADIENT, TemplateBank
    for kind in qi.TRAIN_KINDS:
        od = o.OracleDetector(TemplateBank(T=[5, 8], modalities=[dict(DEFAULT_COLOR_GRADIENT, strong_threshold=qi.TRAIN_STRONG[kind])]))
        bgr, mask = qi.training_view(kind)
        tid, bb = od.add_template([bgr], "obj", mask)
        assert tid == 0 and bb[2] > 100 and bb[3] > 100, (kind, tid, bb)
        assert [len(t[3]) for t in od.get_templates("obj", tid)] == [63, 31]


def test_planted_faults_show_on_a_hostile_image_and_hardly_on_a_scene():
    """A median of rank 11 or 13, and a tenth of the labels taken from the pixel 1 column, 1 row or 3 rows + 52 columns away (the item step
    of the pipelined interior-tile loop): output pixels changed on a 160 x 160 synthetic scene and on a hostile image of the same size.
    Asserted: each misplacement changes at least ten times as many output pixels on the hostile image."""
    bank = synth.make_bank(6, modalities=("DepthNormal",), T=(5, 8), seed=21, size_range=(24.0, 60.0))
    images = (("synthetic scene", np.ascontiguousarray(synth.make_scene(bank, 160, 160, seed=22)[0][0]), None),
              ("hostile image", qi.hostile_depth(160, 160, 1), qi.normal_table("uniform")))
    changed = {}
    for what, depth, lut in images:
        q, pre = o.quantized_normals(depth, 2000, 50, lut)
        cum = qi.window_counts(pre)
        assert np.array_equal(qi.median_of_counts(cum), q)
        c = qi.depth_coverage(pre)
        print("%s 160x160: %.0f %% of the windows unanimous, at most %d distinct values, equal neighbours %.0f %%"
              % (what, 100.0 * c["distinct"][1] / pre.size, int(np.flatnonzero(c["distinct"]).max()), 100 * c["equal_neighbours"]))
        for rank in (11, 13):
            n = int((qi.median_of_counts(cum, rank) != q).sum())
            print("%s, mutant median of rank %d: %d output labels differ" % (what, rank, n))
            changed[what, rank] = n
        for shift in qi.MISPLACEMENTS:
            bad, planted, moved = qi.misplaced(pre, shift)
            n = int((o.median5(bad) != q).sum())
            print("%s, mutant labels from %s away: %d planted, %d labels differ before the median, %d after" % (what, shift, planted, moved, n))
            changed[what, shift] = n
    for shift in qi.MISPLACEMENTS:
        assert changed["hostile image", shift] >= 10 * max(1, changed["synthetic scene", shift]), shift
