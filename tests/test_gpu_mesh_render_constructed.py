"""The rasteriser kernels (csrc/lmx_mesh.hip) on constructed meshes (mesh_cases.constructed_cases): every byte of gray, depth, mask and
rect against meshsynth.render_view, on what two scanned meshes on tile-multiple frames never do -- staging chunks that fill (slot 255), a
wave with 64 hits next to an empty one, a middle chunk without hits, winners at indices 254 .. 257 and in the last short chunk, exact z ties
between triangles of different gray, frames that are no multiple of the 32x8 tile, pixel centres exactly on edges and vertices, slivers,
projections 1e8 px wide, boxes that clamp away, depth at k + 0.5 mm and at its saturation, views with an empty union box or one in the last
partial tile between ordinary views of one call.  That the cases are what they claim is shown on the CPU (test_mesh_raster_host.py).
Then the trainer (lmx_bank_train_mesh) on a mesh whose centre pixel is covered in some views only, and on a view whose level-1 mask is empty."""
import numpy as np
import pytest

import mesh_cases as mc
from linemod_pose_estimation_amd import NativeBank, meshsynth as ms, render_views
from linemod_pose_estimation_amd.bank import TemplateBank
from oracle import oracle as o
from test_gpu_mesh_train import loop_reference, same_bank
from test_gpu_train_sizes import modalities, same_templates

pytestmark = pytest.mark.gpu

F = ms.ENSENSO["fx"]
CASES = mc.constructed_cases()


def gpu_render(tri, cam, views):
    return render_views(tri, views, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], mc.LIGHT)


def case(name):
    return next(c for c in CASES if c[0] == name)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_render_views_equals_meshraster_c_on_constructed_meshes(case):
    """One batched call; calls of the last 1 and 2 views where the case has several."""
    name, tri, cam, views = case
    exp = mc.constructed_expected(name)
    mc.assert_render_equal(gpu_render(tri, cam, views), exp, name)
    for n in (1, 2):
        if n < len(views):
            mc.assert_render_equal(gpu_render(tri, cam, views[-n:]), tuple(e[-n:] for e in exp), (name, n))


@pytest.mark.parametrize("tail", [""] + ["_after_%d" % n for n in mc.ROOF_FILLERS])
def test_roof_orders_differ_on_the_device_where_the_reference_differs(tail):
    """The ridge's z ties: the device's two orders differ from each other exactly where meshraster.c's two orders do (the 33 ridge pixels)."""
    got, exp = [], []
    for order in ("ab", "ba"):
        name, tri, cam, views = case("roof_" + order + tail)
        got.append(gpu_render(tri, cam, views))
        exp.append(mc.constructed_expected(name))
    for k, what in enumerate(("gray", "depth", "mask", "rects")):
        assert np.array_equal(got[0][k] != got[1][k], exp[0][k] != exp[1][k]), what
    ridge = got[0][0] != got[1][0]
    assert ridge.sum() == 33 and ridge[0, mc.ROOF_ROWS[0]:mc.ROOF_ROWS[1] + 1, mc.ROOF_COLUMN].all()


def test_clamped_out_triangles_change_nothing_on_the_device():
    name, tri, cam, views = case("clamped_out_65x17")
    plain = gpu_render(mc.constructed_info()["clamped_plain"], cam, views)
    mc.assert_render_equal(gpu_render(tri, cam, views), plain, name + " vs the plain lattice")


@pytest.mark.parametrize("name", ["batch_chip_75x41", "batch_plane_75x41", "batch_corner_75x45"])
def test_batch_as_one_call_one_by_one_and_reversed(name):
    """Per-view state (validity, union box, silhouette boxes, centre depth) does not leak from a view to its neighbours."""
    _, tri, cam, views = case(name)
    exp = mc.constructed_expected(name)
    whole = gpu_render(tri, cam, views)
    single = [gpu_render(tri, cam, [v]) for v in views]
    single = tuple(np.concatenate([s[k] for s in single]) for k in range(4))
    reverse = tuple(a[::-1] for a in gpu_render(tri, cam, views[::-1]))
    mc.assert_render_equal(single, whole, name + ": one by one vs one call")
    mc.assert_render_equal(reverse, whole, name + ": reversed vs one call")
    mc.assert_render_equal(whole, exp, name)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------

def test_trainer_centre_depth_of_views_that_miss_the_centre():
    """MS_CENTRE_DEPTH per view: the side-car's distances where the centre pixel is covered (D = distance - depth) and where it is not
    (D = distance), a view of the second kind after one of the first; bank, ids and meta equal the per-view loop's."""
    W, H, f = 321, 241, F / 2
    tri, views = mc.off_origin_chip(), ms.view_grid()[11:2652:240]
    assert len(views) == 12
    c = np.asarray([ms.render_view(tri, R, d, f, f, W, H)[1][H // 2, W // 2] for R, d in views])
    D = np.asarray([d - float(np.float32(ci) / np.float32(1000.0)) for (R, d), ci in zip(views, c)])
    ref, ref_ids, ref_meta = loop_reference(tri, views, W, H, f)
    acc = np.nonzero(ref_ids >= 0)[0]
    print("centre depths %s, accepted %s" % (c.tolist(), acc.tolist()))
    assert list(ref_ids) == list(range(12))                 # the oracle trainer's answer, established with the oracle alone
    zero, positive = acc[c[acc] == 0], acc[c[acc] > 0]
    assert len(zero) >= 1 and len(positive) >= 1 and zero.max() > positive.min()
    for device_candidates in (False, True):
        nb = NativeBank.create(ms.empty_bank().T, ms.empty_bank().modalities)
        meta = nb.train_mesh(tri, views, W, H, f, f, device_candidates=device_candidates)
        assert np.array_equal(nb.last_template_ids, ref_ids) and meta == ref_meta
        assert np.array_equal(nb.last_side_car["distances"], D[acc]), (nb.last_side_car["distances"], D[acc])
        same_bank(nb.to_bank(), ref.to_bank())


@pytest.mark.parametrize("nf", [63, 4])
def test_trainer_view_whose_level_1_mask_is_empty(nf):
    """A one-pixel strip in an odd column between two ordinary views of one call: level 1 of its mask (mask(2y, 2x)) is empty, its
    silhouette box there stays unset and mesh_window answers with the 4x4 corner.  Ids and templates equal the oracle's and the per-view
    loop's; the neighbours' templates are those of a call without the strip."""
    tri, cam, views = mc.strip_case()
    W, H, f, cx, cy = cam["width"], cam["height"], cam["fx"], cam["cx"], cam["cy"]
    T, mdesc = (5, 8), modalities(nf)
    od = o.OracleDetector(TemplateBank(T=list(T), modalities=mdesc))
    loop = NativeBank.create(list(T), mdesc)
    ref_ids, loop_ids, ref_meta = [], [], []
    for i, (R, dist) in enumerate(views):
        gray, depth, mask, rect = ms.render_view(tri, R, dist, f, f, W, H, cx, cy)
        if i == 1:
            ys, xs = np.nonzero(mask)
            assert len(xs) >= 10 and set(xs.tolist()) == {161} and rect[2] == 1 and not mask[::2, ::2].any()
        else:
            assert mask[::2, ::2].sum() > 100 * 255
        bgr = np.ascontiguousarray(np.repeat(gray[:, :, None], 3, 2))
        ref_ids.append(od.add_template([bgr, depth], "obj", mask)[0])
        loop_ids.append(loop.add_template([bgr, depth], "obj", mask)[0])
        if ref_ids[-1] >= 0:
            ref_meta.append({"view": i, "rect": rect, "distance": dist})
    assert ref_ids == [0, -1, 1] and loop_ids == ref_ids          # what the oracle gives: the strip is rejected, its neighbours are not
    same_templates(loop.to_bank(), od, 2)
    for device_candidates in (False, True):
        nb = NativeBank.create(list(T), mdesc)
        meta = nb.train_mesh(tri, views, W, H, f, f, cx, cy, device_candidates=device_candidates)
        assert list(nb.last_template_ids) == ref_ids and meta == ref_meta and [m["view"] for m in meta] == [0, 2]
        same_templates(nb.to_bank(), od, 2)
        alone = NativeBank.create(list(T), mdesc)
        alone.train_mesh(tri, [views[0], views[2]], W, H, f, f, cx, cy, device_candidates=device_candidates)
        same_bank(nb.to_bank(), alone.to_bank())
        same_bank(nb.to_bank(), loop.to_bank())
