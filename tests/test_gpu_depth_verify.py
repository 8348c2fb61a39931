"""The depth check of matches on the device (csrc/lmx_verify.hip): the job form of k_walk on constructed crops against the numpy restatement of
tests/depth_verify_cases.py, every integer; the batch form; DepthTemplates.from_mesh (renderer + k_depth_crop) against
meshsynth.render_view; renderer and kernel against each other; the chain train -> match -> depth check -> cluster from Python and from
C++ (tests/cpp/depth_verify_main.cpp).  Integer outputs are compared exactly; nothing here has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

import depth_verify_cases as dvc
import mesh_cases as mc
from conftest import ROOT
from linemod_pose_estimation_amd import (DEPTH_DIFF_DTYPE, MATCH_DTYPE, DepthTemplates, Detector, NativeBank, _lib, cluster_matches_scored, depth_values,
                                         meshsynth as ms)

pytestmark = pytest.mark.gpu

F = ms.ENSENSO["fx"]
W, H = 320, 240


def as_rows(d):
    """DEPTH_DIFF_DTYPE records -> int64 [n, 3] in the restatement's order (sum_abs_mm, n_valid, n_template)."""
    assert d.dtype == DEPTH_DIFF_DTYPE
    return np.stack([d["sum_abs_mm"].astype(np.int64), d["n_valid"].astype(np.int64), d["n_template"].astype(np.int64)], 1)


def assert_rows(got, want, rows=None):
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, [(int(i), None if rows is None else tuple(int(v) for v in rows[i]), got[i].tolist(), want[i].tolist()) for i in bad[:5]]


# ---- constructed crops ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed():
    crops, scene, rows, expected = dvc.constructed()
    t = DepthTemplates.from_crops(crops)
    yield t, crops, scene, rows, expected
    t.close()


def test_constructed_crops_equal_the_restatement(constructed):
    t, crops, scene, rows, expected = constructed
    assert len(t) == len(crops) == len(dvc.WIDTHS) * len(dvc.HEIGHTS)
    for k in (0, 17, len(crops) - 1):
        assert t.rect(k) == (0, 0, crops[k].shape[1], crops[k].shape[0]) and np.array_equal(t.crop(k), crops[k])
    got = as_rows(t.diff(scene, dvc.match_records(MATCH_DTYPE, rows)))
    assert_rows(got, expected, rows)
    # the placement the list is about: a crop cut by the right border must not read on into the next row
    right, without_predicate = 0, 0
    flat = np.concatenate([scene.ravel(), np.zeros(1024, np.uint16)])
    for k, c in enumerate(crops):
        h, w = c.shape
        if w >= 2:
            x, y = dvc.SCENE_W - (w + 1) // 2, 5
            i = int(np.nonzero((rows[:, 0] == x) & (rows[:, 1] == y) & (rows[:, 2] == k))[0][0])
            right += int(got[i, 1])
            without_predicate += sum(int(c[r, j] != 0 and flat[(y + r) * dvc.SCENE_W + x + j] != 0) for r in range(h) for j in range(w))
    assert 0 < right < without_predicate
    far = rows[:, 0] >= dvc.INT32_MAX - 200
    assert far.sum() >= 100 and not got[far, 1].any() and (got[far, 2] == expected[far, 2]).all() and got[far, 2].any()


def test_sum_does_not_wrap_at_2_to_32():
    t = DepthTemplates.from_crops([np.full((256, 257), 65535, np.uint16)])
    d = t.diff(np.ones((300, 300), np.uint16), dvc.match_records(MATCH_DTYPE, [(20, 30, 0)]))
    assert as_rows(d).tolist() == [[65534 * 65792, 65792, 65792]] and 65534 * 65792 == 4311612928 > 2 ** 32
    t.close()


def test_rows_wider_than_one_trip_of_a_wave():
    """Crops of 64, 65 and 138 vectors a row (dvc.WIDE_SIZES): the lanes of a wave take a row's vectors 64 at a time, so 513 pixels are the
    first width at which a lane takes a second trip along its row, and at 1100 some take three."""
    crops, scene, rows, expected = dvc.wide()
    assert [c.shape[::-1] for c in crops] == list(dvc.WIDE_SIZES) and scene.shape == (12, 1200) and len(rows) == 8 * len(crops)
    assert 2 * (expected[:, 1] > 0).sum() >= len(rows)                   # at least half the placements have something to compare
    assert (rows[:, 0] == dvc.INT32_MAX - 1100).any() and (rows[:, 0] < 0).any() and (rows[:, 0] & 1).any()
    t = DepthTemplates.from_crops(crops)
    assert_rows(as_rows(t.diff(scene, dvc.match_records(MATCH_DTYPE, rows))), expected, rows)
    t.close()


def test_batch_offsets_strided_frames_and_class_filter(constructed):
    t, crops, _, _, _ = constructed
    rng = np.random.default_rng(77)
    wide = np.zeros((3, dvc.SCENE_H, dvc.SCENE_W + 13), np.uint16)
    wide[:, :, dvc.SCENE_W:] = 4242                                  # what lies behind a row's end in memory is not the next row
    for f in range(3):
        wide[f, :, :dvc.SCENE_W] = dvc._values(rng, (dvc.SCENE_H, dvc.SCENE_W), 0.2)
    frames = [wide[f, :, :dvc.SCENE_W] for f in range(3)]
    assert not frames[1].flags["C_CONTIGUOUS"] and frames[1].strides[0] == 2 * (dvc.SCENE_W + 13)
    offsets = [0, 0, 7, 19]                                          # the first frame has no matches
    rows = [(int(rng.integers(-20, dvc.SCENE_W)), int(rng.integers(-6, dvc.SCENE_H)), int(rng.integers(0, len(crops)))) for _ in range(19)]
    rows[3] = (dvc.SCENE_W - 30, 5, dvc.WIDTHS.index(63) * len(dvc.HEIGHTS) + 4)      # a 63 x 9 crop across the right border
    m = dvc.match_records(MATCH_DTYPE, rows)
    want = dvc.np_diff_matches(crops, frames, m, offsets)
    assert (want[:7, 1] > 0).any() and (want[7:, 1] > 0).any()
    assert_rows(as_rows(t.diff(frames, m, offsets)), want, np.asarray(rows))
    # the same matches against the other frame give other numbers: the frame index reaches the kernel
    swapped = dvc.np_diff_matches(crops, [frames[0], frames[2], frames[1]], m, offsets)
    assert (swapped != want).any()
    assert_rows(as_rows(t.diff([frames[0], frames[2], frames[1]], m, offsets)), swapped, np.asarray(rows))
    # class filter: the others get zeros and their template ids are not looked at
    m["class_index"] = np.arange(19) % 3
    m["template_id"][m["class_index"] == 2] = len(crops) + 5
    for cls in (0, 1):
        want_c = dvc.np_diff_matches(crops, frames, m, offsets, cls)
        assert (want_c[m["class_index"] != cls] == 0).all() and want_c[m["class_index"] == cls, 2].all()
        assert_rows(as_rows(t.diff(frames, m, offsets, class_index=cls)), want_c)
    with pytest.raises(_lib.LmxError) as e:
        t.diff(frames, m, offsets)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "match 2:" in str(e.value)


def test_buffers_grow_and_are_reused():
    """5, then 5000, then 5 matches on one object; the 5000-match call twice gives identical bytes."""
    crops, scene, _, _ = dvc.constructed()
    t = DepthTemplates.from_crops(crops)
    rng = np.random.default_rng(78)
    rows = np.stack([rng.integers(-40, dvc.SCENE_W + 10, 5000), rng.integers(-12, dvc.SCENE_H + 6, 5000), rng.integers(0, len(crops), 5000)], 1)
    m = dvc.match_records(MATCH_DTYPE, rows)
    want = np.asarray([dvc.np_diff(crops[k], scene, x, y) for x, y, k in rows], np.int64)
    assert_rows(as_rows(t.diff(scene, m[:5])), want[:5], rows)
    big = t.diff(scene, m)
    assert_rows(as_rows(big), want, rows)
    assert_rows(as_rows(t.diff(scene, m[-5:])), want[-5:], rows[-5:])
    assert t.diff(scene, m).tobytes() == big.tobytes()
    other = dvc._values(rng, (40, 50), 0.2)                          # another frame size on the same object
    want_o = np.asarray([dvc.np_diff(crops[k], other, x, y) for x, y, k in rows[:300]], np.int64)
    assert_rows(as_rows(t.diff(other, m[:300])), want_o, rows)
    t.close()


# ---- from_mesh -------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rendered():
    """40 views of the grid at 320 x 240, half the focal length: more than one device batch of 32.  -> (templates, views, host renders)."""
    chip, grid = ms.load_mesh("memoryChip2"), ms.view_grid()
    views = [grid[i] for i in range(3, 2652, 67)][:40]
    assert len(views) == 40
    host = [ms.render_view(chip, R, d, F / 2, F / 2, W, H) for R, d in views]     # (gray, depth, mask, rect)
    t = DepthTemplates.from_mesh(chip, views, W, H, F / 2, F / 2)
    yield t, views, host
    t.close()


def test_from_mesh_rects_and_crops_equal_render_view(rendered):
    t, views, host = rendered
    assert len(t) == 40
    padded = 0
    for i, (_, depth, mask, rect) in enumerate(host):
        x, y, w, h = rect
        assert w > 10 and h > 10 and np.array_equal(depth != 0, mask != 0)        # in these renders depth != 0 is exactly the mask
        assert t.rect(i) == rect, i
        got = t.crop(i)
        assert got.shape == (h, w) and np.array_equal(got, depth[y:y + h, x:x + w]), i
        padded += h * ((w + 7) // 8 * 8) * 2
    # device use: the crops with rows padded to 16 bytes + 24 bytes of table per template -- not 40 frames
    assert padded <= t.device_bytes <= padded + 24 * 40
    assert t.device_bytes < 40 * W * H * 2 // 10


def test_from_mesh_view_outside_gives_an_empty_crop():
    name, tri, cam, views = [c for c in mc.cases() if c[0].endswith("_outside")][0]
    t = DepthTemplates.from_mesh(tri, views, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    assert len(t) == 1 and t.rect(0) == (0, 0, 0, 0) and t.crop(0).shape == (0, 0) and t.device_bytes == 24
    scene = np.full((cam["height"], cam["width"]), 700, np.uint16)
    d = t.diff(scene, dvc.match_records(MATCH_DTYPE, [(10, 10, 0), (-5, 300, 0), (0, 0, 0)]))
    assert not as_rows(d).any()
    t.close()


def test_from_mesh_invalid_view_fails_with_its_index():
    chip, grid = ms.load_mesh("memoryChip2"), ms.view_grid()
    views = [grid[i] for i in range(3, 2652, 67)][:40]
    R_bad = mc.view_reaching_behind(chip, grid, 0.02)
    with pytest.raises(_lib.LmxError) as e:
        DepthTemplates.from_mesh(chip, views[:35] + [(R_bad, 0.02)] + views[35:], W, H, F / 2, F / 2)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "view 35 " in str(e.value)


def test_renderer_and_kernel_agree(rendered):
    """A view's own render as the scene, the match at its rect origin: no difference, every covered pixel valid; the scene 7 mm further
    away wherever it has a value: 7 mm per pixel."""
    t, views, host = rendered
    frames, rows = [], []
    for v in (0, 13, 31, 32, 39):
        _, depth, mask, rect = host[v]
        frames += [depth, np.where(depth != 0, depth + 7, 0).astype(np.uint16)]
        rows += [(rect[0], rect[1], v)] * 2
    d = t.diff(frames, dvc.match_records(MATCH_DTYPE, rows), list(range(len(frames) + 1)))
    for k, v in enumerate((0, 13, 31, 32, 39)):
        covered = int(np.count_nonzero(host[v][2]))
        same, further = d[2 * k], d[2 * k + 1]
        assert covered > 500 and same["sum_abs_mm"] == 0 and same["n_valid"] == same["n_template"] == covered, (v, same, covered)
        assert further["n_valid"] == further["n_template"] == covered and further["sum_abs_mm"] == 7 * covered, (v, further, covered)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------

THRESHOLD = 75.0


@pytest.fixture(scope="module")
def trained():
    """A 204-view bank of the chip at 320 x 240, a two-instance scene, its matches at a threshold that yields a few hundred."""
    chip, cpu = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary")
    views = ms.view_grid()[:204]
    b = ms.empty_bank()
    nb = NativeBank.create(b.T, b.modalities)
    meta = nb.train_mesh(chip, views, W, H, F / 2, F / 2)
    sc = nb.last_side_car
    assert len(meta) == len(sc["rects"]) > 100
    sources, truth = ms.make_scene(chip, views, width=W, height=H, seed=11, n_instances=2, fx=F / 2, fy=F / 2, other_tri=cpu, n_other=1, margin=44)
    det = Detector(nb, W, H)
    matches = det.match(sources, THRESHOLD)
    det.close()
    template_views = list(zip(sc["R"], sc["T"][:, 2]))
    t = DepthTemplates.from_mesh(chip, template_views, W, H, F / 2, F / 2)
    yield chip, views, sc, sources, matches, t
    t.close()


def test_end_to_end_diff_equals_the_restatement_and_clusters(trained):
    chip, views, sc, sources, matches, t = trained
    assert 100 < len(matches) < 2000, len(matches)
    assert len(t) == len(sc["rects"]) and all(t.rect(i) == tuple(sc["rects"][i]) for i in range(0, len(t), 9))
    crops = {int(k): t.crop(int(k)) for k in np.unique(matches["template_id"])}
    for k in list(crops)[:6]:                       # the crops are the trainer's views: render_view of the side-car's pose
        x, y, w, h = t.rect(k)
        assert np.array_equal(crops[k], ms.render_view(chip, sc["R"][k], sc["T"][k, 2], F / 2, F / 2, W, H)[1][y:y + h, x:x + w])
    d = t.diff(sources[1], matches)
    want = np.asarray([dvc.np_diff(crops[int(m["template_id"])], sources[1], int(m["x"]), int(m["y"])) for m in matches], np.int64)
    assert_rows(as_rows(d), want)
    assert (want[:, 1] > 0).all() and (want[:, 1] < want[:, 2]).any() and (want[:, 0] > 0).all()     # scene holes; no match is the render itself
    values = depth_values(d)
    assert np.isfinite(values).all() and (values < 0).all()
    clusters, members = cluster_matches_scored(matches, values, sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
    assert len(clusters) >= 1 and (np.diff(clusters["score"]) <= 0).all()
    for c in clusters:
        mem = members[c["member_begin"]:c["member_begin"] + c["member_count"]]
        assert c["member_count"] > 2 and ((mem >= 0) & (mem < len(matches))).all()
        total = 0.0
        for v in values[mem]:
            total += float(v)
        assert c["score"] == total / len(mem)          # the mean in voting order


def test_cpp_caller_runs_the_same_chain(trained, tmp_path):
    """tests/cpp/depth_verify_main.cpp (lmx::linemod::DepthTemplates + lmx_cluster_matches_scored) prints what the Python path computes."""
    chip, views, sc, sources, matches, t = trained
    exe = str(tmp_path / "depth_verify_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "depth_verify_main.cpp"),
                           "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    np.ascontiguousarray(chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(views).tofile(tmp_path / "views.f64")
    np.ascontiguousarray(sources[0]).tofile(tmp_path / "bgr.u8")
    np.ascontiguousarray(sources[1]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(W), str(H), repr(F / 2), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(THRESHOLD)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    d = t.diff(sources[1], matches)
    clusters, _ = cluster_matches_scored(matches, depth_values(d), sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
    want = ["templates %d depth_templates %d device_bytes %d" % (len(sc["rects"]), len(t), t.device_bytes),
            "matches %d sum_abs_mm %d n_valid %d" % (len(matches), d["sum_abs_mm"].sum(), d["n_valid"].sum())]
    want += ["cluster %d %d %d rect %d %d %d %d members %d mean_depth_difference_mm %.17g" % (tuple(c["index"]) + tuple(c["rect"]) + (c["member_count"], -1000.0 * c["score"]))
             for c in clusters]
    assert len(clusters) >= 1 and res.stdout.strip().splitlines() == want
