"""The normal term of a match on the device (csrc/lmx_verify.hip: k_normal_map_frames, k_normal_map_crops, the NORMALS
forms of k_walk; csrc/lmx_f2.hip: the third form of k_f2_finalize_cluster) against the CPU build of the shared header and the numpy
restatement of tests/normal_verify_cases.py.  Every output is integer or compared bit for bit; nothing here has a tolerance."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import cluster_cases as cc
import depth_verify_cases as dvc
import mesh_cases as mc
import normal_verify_cases as nvc
from conftest import ROOT
from linemod_pose_estimation_amd import (DEPTH_DIFF_DTYPE, MATCH_DTYPE, NORMAL_DIFF_DTYPE, DepthTemplates, Detector, NativeBank, _lib, cluster_matches_scored,
                                         depth_values, meshsynth as ms, normal_angle_table, normal_values, synth)
from oracle import oracle as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return nvc.build_host_lib(tmp_path_factory.mktemp("nvhost"))


def strided(frames, pad=5, fill=4242):
    """The same images as views whose rows are `pad` elements further apart, with `fill` behind each row's end."""
    out = []
    for f in frames:
        wide = np.full((f.shape[0], f.shape[1] + pad), fill, np.uint16)
        wide[:, :f.shape[1]] = f
        out.append(wide[:, :f.shape[1]])
    return out


def n_rows(nd):
    assert nd.dtype == NORMAL_DIFF_DTYPE and not nd["reserved"].any()
    return np.stack([nd["sum_angle_urad"].astype(np.int64), nd["n_normal"].astype(np.int64)], 1)


def d_rows(d):
    return np.stack([d["sum_abs_mm"].astype(np.int64), d["n_valid"].astype(np.int64), d["n_template"].astype(np.int64)], 1)


def np_both(crops, crop_normals, frames, frame_normals, matches, offsets, table, class_index=-1):
    """The restatement over a match list -> int64 [n, 5] (sum_abs_mm, n_valid, n_template, sum_angle_urad, n_normal); zeros for another class."""
    out = np.zeros((len(matches), 5), np.int64)
    for f in range(len(frames)):
        for i in range(int(offsets[f]), int(offsets[f + 1])):
            m = matches[i]
            if class_index >= 0 and int(m["class_index"]) != class_index:
                continue
            k = int(m["template_id"])
            if crops[k].size:
                out[i] = nvc.np_normal_diff(crops[k], crop_normals[k], frames[f], frame_normals[f], int(m["x"]), int(m["y"]), table)
    return out


# ---- 1. the scene's normal map --------------------------------------------------------------------------------------------------------------------

def test_scene_normal_map_equals_the_host_header(host):
    """11 = 2 * 5 + 1 is the first size with a pixel whose taps all lie inside; the others straddle the workgroup's 256 pixels and the
    widths of vector accesses.  Two frames per upload, rows strided."""
    t = DepthTemplates.from_crops([np.ones((3, 3), np.uint16)])
    t.enable_normals(nvc.FX, nvc.FY)
    by = dict(nvc.constructed_images())
    valid = 0
    for w in (11, 12, 64, 65, 70):
        for h in (11, 13, 37):
            a = by["scene %dx%d" % (w, h)]
            b = np.ascontiguousarray(a[::-1, ::-1])
            frames = strided([a, b])
            assert not frames[0].flags["C_CONTIGUOUS"]
            t.upload_scene(frames)
            for f, img in enumerate((a, b)):
                got = t.debug_scene_normals(f)
                want = nvc.host_map(host, img)
                assert got.shape == (h, w, 4) and np.array_equal(got, want), (w, h, f)
                valid += int(want[..., 3].sum())
    assert valid > 5000
    # other parameters reach the kernel
    t.enable_normals(500.0, 1100.0, difference_threshold=20, distance_threshold=940)
    img = by["scene 70x37"]
    t.upload_scene(img)
    want = nvc.host_map(host, img, 500.0, 1100.0, 20, 940)
    assert np.array_equal(t.debug_scene_normals(0), want) and not np.array_equal(want, nvc.host_map(host, img))
    t.close()


# ---- 2. the crops' normal maps ---------------------------------------------------------------------------------------------------------------------

def make_crops(seed=5):
    """One crop per (width, height) of the depth check's list: a surface in front of the distance threshold, a tenth holes.  Up to five
    rows no pixel has a tap above or below it, so no normal; a few taller crops follow the list."""
    rng = np.random.default_rng(seed)
    sizes = [(w, h) for w in dvc.WIDTHS for h in dvc.HEIGHTS] + [(w, h) for w in (9, 63, 65, 129) for h in (12, 23)]
    return [nvc.scene_image(w, h, rng) for w, h in sizes]


def test_crop_normal_maps_equal_the_host_header(host):
    """The crops' rows are padded to 8 elements on the device: a tap that falls into the padding is a tap outside the crop, and the
    padding's own normals are never handed out -- get_normals equals the header's map of the unpadded crop."""
    crops = make_crops() + [np.zeros((0, 0), np.uint16), nvc.opposed_planes()[0]]
    t = DepthTemplates.from_crops(crops)
    before = t.device_bytes
    with pytest.raises(_lib.LmxError):
        t.normals(0)
    t.enable_normals(nvc.FX, nvc.FY)
    padded = sum(c.shape[0] * ((c.shape[1] + 7) // 8 * 8) for c in crops)
    assert len(crops) >= len(dvc.WIDTHS) * len(dvc.HEIGHTS) + 2 and before == 2 * padded + 24 * len(crops)
    assert t.device_bytes - before == 8 * padded + 8 * len(crops)       # 8 bytes per stored element, one address per template
    valid = 0
    for k, c in enumerate(crops):
        got = t.normals(k)
        assert got.shape == c.shape + (4,) and np.array_equal(got, nvc.host_map(host, c) if c.size else got), (k, c.shape)
        valid += int(got[..., 3].sum())
        assert np.array_equal(t.crop(k), c)
    assert valid > 3000
    t.enable_normals(nvc.FX, nvc.FY, difference_threshold=9)             # a second call with other parameters recomputes
    k = len(crops) - 3
    want = nvc.host_map(host, crops[k], diff_t=9)
    assert np.array_equal(t.normals(k), want) and not np.array_equal(want, nvc.host_map(host, crops[k]))
    assert t.device_bytes - before == 8 * padded + 8 * len(crops)
    t.close()


# ---- 3. both diffs of constructed matches ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed():
    crops = make_crops()
    rng = np.random.default_rng(6)
    frames = [nvc.scene_image(dvc.SCENE_W, dvc.SCENE_H, rng) for _ in range(3)]
    t = DepthTemplates.from_crops(crops)
    t.enable_normals(nvc.FX, nvc.FY)
    plain = DepthTemplates.from_crops(crops)         # the twin that never enables normals
    s = SimpleNamespace(crops=crops, frames=frames, t=t, plain=plain, crop_normals=[nvc.np_normal_map(c) for c in crops],
                        frame_normals=[nvc.np_normal_map(f) for f in frames], table=normal_angle_table())
    yield s
    t.close()
    plain.close()


def test_constructed_matches_equal_the_restatement(constructed):
    s = constructed
    rows = [(x, y, k) for k, c in enumerate(s.crops) for (x, y) in dvc.positions(c.shape[1], c.shape[0])]
    # three frames with uneven offsets: the crops' placements go to frame 0, 1, 2 in turn, sorted by frame
    rows.sort(key=lambda r: (r[2] * 7 + r[0]) % 3)
    frame_of = np.asarray([(r[2] * 7 + r[0]) % 3 for r in rows])
    offsets = [0] + [int((frame_of <= f).sum()) for f in range(3)]
    assert len(set(np.diff(offsets))) == 3
    m = dvc.match_records(MATCH_DTYPE, rows)
    want = np_both(s.crops, s.crop_normals, s.frames, s.frame_normals, m, offsets, s.table)
    outside = want[:, 1] == 0
    assert (want[:, 4] > 0).sum() > 200 and outside.sum() > 200 and not want[outside, 3:].any()
    assert ((want[:, 4] < want[:, 1]) & (want[:, 4] > 0)).any()                     # holes and far pixels: fewer normals than depths
    frames = strided(s.frames)
    dd, nd = s.t.normal_diff(frames, m, offsets)
    bad = np.nonzero((np.concatenate([d_rows(dd), n_rows(nd)], 1) != want).any(1))[0]
    assert len(bad) == 0, [(rows[i], d_rows(dd)[i].tolist(), n_rows(nd)[i].tolist(), want[i].tolist()) for i in bad[:5]]
    assert dd.tobytes() == s.plain.diff(frames, m, offsets).tobytes() == s.t.diff(frames, m, offsets).tobytes()
    # the frame index reaches the kernel
    swapped = [frames[1], frames[2], frames[0]]
    _, nd2 = s.t.normal_diff(swapped, m, offsets)
    want2 = np_both(s.crops, s.crop_normals, [s.frames[1], s.frames[2], s.frames[0]], [s.frame_normals[1], s.frame_normals[2], s.frame_normals[0]], m, offsets, s.table)
    assert np.array_equal(n_rows(nd2), want2[:, 3:]) and not np.array_equal(want2, want)
    # class filter: the others get zeros and their template ids are not looked at
    m["class_index"] = np.arange(len(m)) % 3
    m["template_id"][m["class_index"] == 2] = len(s.crops) + 5
    want_c = np_both(s.crops, s.crop_normals, s.frames, s.frame_normals, m, offsets, s.table, class_index=1)
    dd, nd = s.t.normal_diff(frames, m, offsets, class_index=1)
    assert np.array_equal(np.concatenate([d_rows(dd), n_rows(nd)], 1), want_c) and want_c[:, 4].any() and not want_c[m["class_index"] != 1].any()
    with pytest.raises(_lib.LmxError) as e:
        s.t.normal_diff(frames, m, offsets)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "match" in str(e.value)
    with pytest.raises(_lib.LmxError) as e:
        s.plain.normal_diff(frames, m, offsets, class_index=1)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "enable_normals" in str(e.value)


def test_holes_in_the_scene_and_in_the_crop(constructed):
    s = constructed
    k = dvc.WIDTHS.index(65) * len(dvc.HEIGHTS) + 4
    crop, frame = s.crops[k], s.frames[0]
    assert (crop == 0).any() and (frame[7:16, 10:75] == 0).any()
    dd, nd = s.t.normal_diff(frame, dvc.match_records(MATCH_DTYPE, [(10, 7, k)]))
    want = nvc.np_normal_diff(crop, s.crop_normals[k], frame, s.frame_normals[0], 10, 7, s.table)
    assert d_rows(dd)[0].tolist() + n_rows(nd)[0].tolist() == list(want) and 0 < want[4] < want[1] < want[2] < crop.size


def test_rows_wider_than_one_trip_of_a_wave():
    """Crops of 64, 65 and 138 vectors a row (dvc.WIDE_SIZES): up to one, two and three trips of a wave's 64 lanes along a row, with the
    crop's normals read next to its depths on every trip.  nvc.wide() says where crops this flat get their normals from."""
    crops, crop_normals, scene, scene_normals, rows = nvc.wide()
    table = normal_angle_table()
    want = np.asarray([nvc.np_normal_diff(crops[k], crop_normals[k], scene, scene_normals, x, y, table) for x, y, k in rows], np.int64)
    assert [c.shape[::-1] for c in crops] == list(dvc.WIDE_SIZES) and scene.shape == (12, 1200) and len(rows) == 8 * len(crops)
    assert 2 * (want[:, 1] > 0).sum() >= len(rows) and 2 * (want[:, 4] > 0).sum() >= len(rows)     # half the placements count in each term
    t = DepthTemplates.from_crops(crops)
    t.enable_normals(nvc.FX, nvc.FY)
    for k, n in enumerate(crop_normals):
        assert np.array_equal(t.normals(k), n), k
    m = dvc.match_records(MATCH_DTYPE, rows)
    dd, nd = t.normal_diff(scene, m)
    got = np.concatenate([d_rows(dd), n_rows(nd)], 1)
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, [(rows[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    assert dd.tobytes() == t.diff(scene, m).tobytes()
    t.close()


# ---- 4. no 32-bit wrap ---------------------------------------------------------------------------------------------------------------------------------

def test_angle_sum_does_not_wrap_at_2_to_32():
    up, down = nvc.opposed_planes()
    t = DepthTemplates.from_crops([up])
    t.enable_normals(nvc.FX, nvc.FY)
    scene = np.zeros((80, 90), np.uint16)
    scene[9:73, 13:77] = down
    # the scene's normals at the patch's border see the zeros around it, as the crop's see the crop's end: the same taps drop out
    dd, nd = t.normal_diff(scene, dvc.match_records(MATCH_DTYPE, [(13, 9, 0)]))
    want = nvc.np_normal_diff(up, nvc.np_normal_map(up), scene, nvc.np_normal_map(scene), 13, 9, normal_angle_table())
    assert d_rows(dd)[0].tolist() + n_rows(nd)[0].tolist() == list(want)
    assert want[4] == 64 * 64 and want[3] > 2 ** 32
    t.close()


# ---- 7. existing behaviour untouched ------------------------------------------------------------------------------------------------------------------

def test_diff_on_an_object_with_normals_equals_its_twin_without(constructed):
    s = constructed
    rng = np.random.default_rng(8)
    rows = np.stack([rng.integers(-40, dvc.SCENE_W + 10, 600), rng.integers(-12, dvc.SCENE_H + 6, 600), rng.integers(0, len(s.crops), 600)], 1)
    m = dvc.match_records(MATCH_DTYPE, rows)
    a = s.t.diff(s.frames[1], m)
    assert a.tobytes() == s.plain.diff(s.frames[1], m).tobytes() and (a["n_valid"] > 0).sum() > 100
    assert s.plain.device_bytes == 2 * sum(c.shape[0] * ((c.shape[1] + 7) // 8 * 8) for c in s.crops) + 24 * len(s.crops)


# ---- 5. the term does its job ------------------------------------------------------------------------------------------------------------------------

F = ms.ENSENSO["fx"]
W, H = 320, 240
THRESHOLD = 75.0


def near(cluster, pos):
    return abs(int(cluster["rect"][0]) - pos[0]) <= 10 and abs(int(cluster["rect"][1]) - pos[1]) <= 10


def test_the_normal_term_tells_the_object_from_a_wall():
    """One rendered template twice in one frame: at A the object itself, 6 mm further away; at B a fronto-parallel plane at the template's
    mean depth under the same silhouette, whose mean absolute depth difference is below 6 mm (the chip is 2.6 mm thick and lies nearly
    flat in this view).  The depth score prefers the wall; with the normal term the object comes first."""
    chip = ms.load_mesh("memoryChip2")
    R, dist = ms.view_grid()[582]
    b = ms.empty_bank(modalities=("ColorGradient",))
    nb = NativeBank.create(b.T, b.modalities)
    nb.train_mesh(chip, [(R, dist)], W, H, F / 2, F / 2)
    sc = nb.last_side_car
    assert len(sc["rects"]) == 1
    gray, depth, _, (x, y, w, h) = ms.render_view(chip, R, dist, F / 2, F / 2, W, H)
    crop, g = depth[y:y + h, x:x + w], gray[y:y + h, x:x + w]
    on = crop != 0
    mean = int(round(float(crop[on].mean())))
    A, B = (20, 30), (190, 30)      # side by side: the reference's computeIoU takes two boxes apart in BOTH axes for overlapping ones
    bgr, scene = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint16)
    for (px, py), d in ((A, np.where(on, crop + 6, 0)), (B, np.where(on, mean, 0))):
        bgr[py:py + h, px:px + w] = g[:, :, None]
        scene[py:py + h, px:px + w] = d
    # what was built, by the restatement with the crop laid exactly over each paste: 6 mm everywhere at A, less than 6 mm on average at B
    table = normal_angle_table()
    cn, sn = nvc.np_normal_map(crop, F / 2, F / 2), nvc.np_normal_map(scene, F / 2, F / 2)
    at_a = nvc.np_normal_diff(crop, cn, scene, sn, A[0], A[1], table)
    at_b = nvc.np_normal_diff(crop, cn, scene, sn, B[0], B[1], table)
    assert at_a[0] == 6 * at_a[1] and at_a[1] == at_b[1] == int(on.sum()) and at_b[0] < 6 * at_b[1]
    assert at_a[4] > 1000 and at_b[4] > 1000 and at_a[3] / at_a[4] < 0.05e6 < 0.2e6 < at_b[3] / at_b[4]       # mean angles: under 0.05 rad, over 0.2 rad

    t = DepthTemplates.from_mesh(chip, list(zip(sc["R"], sc["T"][:, 2])), W, H, F / 2, F / 2)
    t.enable_normals(F / 2, F / 2)
    assert t.rect(0) == (x, y, w, h)
    det = Detector(nb, W, H)
    det.set_cluster_sidecar(sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 0)
    det.upload([[bgr]])
    det.enqueue(1, 95.0)
    det.enqueue(1, 95.0)
    t.upload_scene(scene)
    m, d, c_depth, _ = det.collect_clusters_depth(1, t)[0]
    t.upload_scene(scene)
    m2, d2, nd2, c_normal, _ = det.collect_clusters_depth_normal(1, t)[0]
    assert m.tobytes() == m2.tobytes() and d.tobytes() == d2.tobytes() and len(m) >= 2
    # a match lies at the corner of the template's feature box, a few pixels off the silhouette box's, and the crop is laid at the match
    # as the reference lays it: every match near A and near B still has the wall nearer in depth (below 6 mm) and further in angle
    got = np.concatenate([d_rows(d), n_rows(nd2)], 1)
    values = {}
    for name, pos in (("A", A), ("B", B)):
        idx = [i for i, r in enumerate(m) if abs(int(r["x"]) - pos[0]) <= 8 and abs(int(r["y"]) - pos[1]) <= 8]
        assert len(idx) >= 1, (name, m[["x", "y"]].tolist()[:10])
        for i in idx:
            want = nvc.np_normal_diff(crop, cn, scene, sn, int(m["x"][i]), int(m["y"][i]), table)
            assert got[i].tolist() == list(want), (name, i)
        values[name] = [(got[i, 0] / got[i, 1], nvc.np_value(got[i, 0], got[i, 1], got[i, 3], got[i, 4], -np.inf)) for i in idx]
    assert len(values["A"]) + len(values["B"]) == len(m)
    assert max(mm for mm, _ in values["B"]) < 6.0 and max(mm for mm, _ in values["B"]) < min(mm for mm, _ in values["A"])     # mean |difference| in mm
    assert min(v for _, v in values["A"]) > max(v for _, v in values["B"])                                                  # lmx_match_value
    assert len(c_depth) >= 2 and len(c_normal) >= 2
    assert near(c_depth[0], B) and any(near(c, A) for c in c_depth[1:])
    assert near(c_normal[0], A) and any(near(c, B) for c in c_normal[1:])
    t.close()
    det.close()


# ---- 6. the device chain equals the composition ---------------------------------------------------------------------------------------------------------

def values_of(dd, nd, no_value):
    v = normal_values(dd, nd)
    v[(dd["n_valid"] <= 0) | (nd["n_normal"] <= 0)] = no_value
    return v


def assert_frame_equals_composition(got, matches, dd, nd, clusters, members, what):
    m, d, n, c, mem = got
    assert len(m) == len(matches), (what, len(m), len(matches))
    for k in cc.FIELDS:
        assert np.array_equal(m[k], matches[k]), (what, k)
    assert d.tobytes() == dd.tobytes() and n.tobytes() == nd.tobytes(), what
    assert len(c) == len(clusters), (what, len(c), len(clusters))
    for k in ("index", "rect", "member_count"):
        assert np.array_equal(c[k], clusters[k]), (what, k)
    assert c["score"].tobytes() == clusters["score"].tobytes(), what
    for a, b in zip(c, clusters):
        assert np.array_equal(mem[a["member_begin"]:a["member_begin"] + a["member_count"]], members[b["member_begin"]:b["member_begin"] + b["member_count"]]), what


def composition(t, per_frame, depth, side_car, class_index=-1, no_value=-np.inf):
    """collect's matches through DepthTemplates.normal_diff + cluster_matches_scored -> per frame (matches, ddiffs, ndiffs, clusters, members)."""
    dists, rects, params = side_car
    flat = np.concatenate(per_frame)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in per_frame])])
    dd, nd = t.normal_diff(depth, flat, offsets, class_index=class_index)
    out = []
    for f in range(len(per_frame)):
        a, b = dd[offsets[f]:offsets[f + 1]], nd[offsets[f]:offsets[f + 1]]
        c, mem = cluster_matches_scored(per_frame[f], values_of(a, b, no_value), dists, rects, *params)
        out.append((per_frame[f], a, b, c, mem))
    return out


@pytest.fixture(scope="module")
def trained():
    """The bank of test_gpu_depth_verify.py's `trained` fixture (204 views of the chip at 320 x 240), three two-instance scenes, the
    templates' depth renders with normals, a twin without, and a context with the side-car."""
    chip, cpu = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary")
    views = ms.view_grid()[:204]
    b = ms.empty_bank()
    nb = NativeBank.create(b.T, b.modalities)
    nb.train_mesh(chip, views, W, H, F / 2, F / 2)
    sc = nb.last_side_car
    frames = [ms.make_scene(chip, views, width=W, height=H, seed=seed, n_instances=2, fx=F / 2, fy=F / 2, other_tri=cpu, n_other=1, margin=44)[0] for seed in (11, 12, 13)]
    det = Detector(nb, W, H, max_batch=3)
    det.set_cluster_sidecar(sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
    template_views = list(zip(sc["R"], sc["T"][:, 2]))
    t = DepthTemplates.from_mesh(chip, template_views, W, H, F / 2, F / 2)
    t.enable_normals(F / 2, F / 2)
    plain = DepthTemplates.from_mesh(chip, template_views, W, H, F / 2, F / 2)
    yield SimpleNamespace(chip=chip, views=views, sc=sc, frames=frames, det=det, t=t, plain=plain, side_car=(sc["obj_origin_dists"], sc["rects"], (10, 0.4, 0.05, 2)))
    t.close()
    plain.close()
    det.close()


@pytest.mark.parametrize("class_index,no_value", [(-1, -np.inf), (0, -2.5), (1, -np.inf)])
def test_device_chain_equals_the_composition(trained, class_index, no_value):
    tr = trained
    depth = [fr[1] for fr in tr.frames]
    tr.det.upload(tr.frames)
    tr.det.enqueue(3, THRESHOLD)
    tr.det.enqueue(3, THRESHOLD)
    want = composition(tr.t, tr.det.collect(3), depth, tr.side_car, class_index, no_value)
    tr.t.upload_scene(depth)
    got = tr.det.collect_clusters_depth_normal(3, tr.t, class_index=class_index, no_value=no_value)
    for f in range(3):
        assert_frame_equals_composition(got[f], *want[f], what=f)
    m, dd, nd, c, _ = want[0]
    assert 100 < len(m) < 2000 and len(want[1][0]) > 0 and len(want[2][0]) > 0 and len(c) >= 1
    if class_index == 1:          # the bank has one class: nothing is this class's, every value is no_value
        assert not dd["n_template"].any() and not nd["n_normal"].any() and (c["score"] == no_value).all()
    else:
        assert (nd["n_normal"] > 0).mean() > 0.9 and (nd["n_normal"] <= dd["n_valid"]).all() and (nd["sum_angle_urad"] > 0).any()
        assert (c["score"] < 0).all()
        assert want[0][2].tobytes() != want[1][2].tobytes()
        # the normal term changes the scores: the depth-scored call on the same enqueue's twin gives other numbers
        by_depth, _ = cluster_matches_scored(m, depth_values(dd), *tr.side_car[:2], *tr.side_car[2])
        assert not np.array_equal(np.sort(by_depth["score"]), np.sort(c["score"]))


def test_a_frame_beyond_2048_records_is_finished_on_the_host_with_both_terms():
    """The configuration of test_gpu_cluster_depth.py's fallback test: frame 0 leaves more than 2048 raw records (asserted on the oracle's
    count) and is finished on the host inside the call, frame 1 takes the device chain; both equal the composition."""
    S = 160
    thr, n_t = 45.0, 80
    bank = synth.make_bank(n_t, seed=91, size_range=(20.0, 36.0))
    frames = [synth.make_scene(bank, S, S, seed=94)[0], synth.make_scene(bank, S, S, seed=93, n_instances=1)[0]]
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(n_t) % 4) + rng.uniform(-0.005, 0.005, n_t)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    crops = [nvc.scene_image(int(r[2]), int(r[3]), rng) for r in rects]
    depth = [nvc.scene_image(S, S, rng) for _ in range(2)]          # surfaces the normal term has something to say about
    od = o.OracleDetector(bank)
    sizes = []
    for f in range(2):
        od.match(frames[f], thr)
        sizes.append(len(od.last_raw()))
    assert sizes[0] > cc.F2_MAX > sizes[1] > 0, sizes
    t = DepthTemplates.from_crops(crops)
    t.enable_normals(nvc.FX, nvc.FY)
    det = Detector(bank, S, S, max_batch=2, max_candidates=1 << 17)
    det.set_cluster_sidecar(dists, rects, 10, 0.5, 0.1, 2)
    det.upload(frames)
    det.enqueue(2, thr)
    det.enqueue(2, thr)
    per_frame = det.collect(2, cap_total=1 << 17)
    want = composition(t, per_frame, depth, (dists, rects, (10, 0.5, 0.1, 2)))
    t.upload_scene(depth)
    got = det.collect_clusters_depth_normal(2, t, cap_total=1 << 17)
    table = normal_angle_table()
    cn = [nvc.np_normal_map(c) for c in crops]
    for f in range(2):
        assert_frame_equals_composition(got[f], *want[f], what=f)
        m, dd, nd, c, _ = want[f]
        assert len(c) > 0 and (nd["n_normal"] > 0).any()
        sn = nvc.np_normal_map(depth[f])
        for i in range(0, len(m), max(1, len(m) // 40)):             # and the composition itself is the restatement's
            k = int(m["template_id"][i])
            r = nvc.np_normal_diff(crops[k], cn[k], depth[f], sn, int(m["x"][i]), int(m["y"][i]), table)
            assert d_rows(dd)[i].tolist() + n_rows(nd)[i].tolist() == list(r), (f, i)
    t.close()
    det.close()


def test_refusal_without_normals_leaves_the_enqueue_outstanding(trained):
    tr = trained
    depth = [fr[1] for fr in tr.frames]
    tr.det.upload(tr.frames)
    tr.det.enqueue(3, THRESHOLD)
    tr.plain.upload_scene(depth)
    with pytest.raises(_lib.LmxError) as e:
        tr.det.collect_clusters_depth_normal(3, tr.plain)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "enable_normals" in str(e.value)
    with pytest.raises(_lib.LmxError) as e:
        tr.det.collect_clusters_depth_normal(3, tr.t, no_value=float("nan"))
    assert "not a number" in str(e.value)
    tr.t.upload_scene(depth[:2])
    with pytest.raises(_lib.LmxError) as e:
        tr.det.collect_clusters_depth_normal(3, tr.t)
    assert "holds 2 frames" in str(e.value)
    tr.t.upload_scene(depth)
    got = tr.det.collect_clusters_depth_normal(3, tr.t)       # the enqueue is still there
    assert len(got) == 3 and len(got[0][0]) > 100
    with pytest.raises(_lib.LmxError):                         # and now it is gone
        tr.det.collect_clusters_depth_normal(3, tr.t)


# ---- 7. existing behaviour untouched, on the rendered bank ------------------------------------------------------------------------------------------------

def test_depth_scored_clusters_equal_the_twin_without_normals(trained):
    tr = trained
    depth = [fr[1] for fr in tr.frames]
    tr.det.upload(tr.frames)
    out = []
    for templates in (tr.t, tr.plain):
        tr.det.enqueue(3, THRESHOLD)
        templates.upload_scene(depth)
        out.append(tr.det.collect_clusters_depth(3, templates))
    for f in range(3):
        (m0, d0, c0, mem0), (m1, d1, c1, mem1) = out[0][f], out[1][f]
        assert m0.tobytes() == m1.tobytes() and d0.tobytes() == d1.tobytes() and len(c0) == len(c1) >= 1
        for k in ("index", "rect", "score", "member_begin", "member_count"):
            assert c0[k].tobytes() == c1[k].tobytes(), (f, k)
        assert np.array_equal(mem0[:int(c0["member_count"].sum())], mem1[:int(c1["member_count"].sum())])
    flat = np.concatenate([m for m, _, _, _ in out[0]])
    offsets = np.concatenate([[0], np.cumsum([len(m) for m, _, _, _ in out[0]])])
    assert tr.t.diff(depth, flat, offsets).tobytes() == tr.plain.diff(depth, flat, offsets).tobytes()
    assert tr.t.device_bytes > 4 * tr.plain.device_bytes


# ---- 8. the C++ caller -----------------------------------------------------------------------------------------------------------------------------------

def test_cpp_caller_prints_what_the_python_path_computes(trained, tmp_path):
    tr = trained
    exe = str(tmp_path / "normal_verify_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "normal_verify_main.cpp"),
                           "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    sources = tr.frames[0]
    np.ascontiguousarray(tr.chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(tr.views).tofile(tmp_path / "views.f64")
    np.ascontiguousarray(sources[0]).tofile(tmp_path / "bgr.u8")
    np.ascontiguousarray(sources[1]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(W), str(H), repr(F / 2), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(THRESHOLD)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    tr.det.upload([sources])
    tr.det.enqueue(1, THRESHOLD)
    tr.t.upload_scene(sources[1])
    m, d, nd, clusters, _ = tr.det.collect_clusters_depth_normal(1, tr.t)[0]
    want = ["templates %d depth_templates %d device_bytes %d" % (len(tr.sc["rects"]), len(tr.t), tr.t.device_bytes),
            "matches %d sum_abs_mm %d n_valid %d sum_angle_urad %d n_normal %d" % (len(m), d["sum_abs_mm"].sum(), d["n_valid"].sum(), nd["sum_angle_urad"].sum(), nd["n_normal"].sum()),
            "first value %.17g" % normal_values(d[:1], nd[:1])[0]]
    want += ["cluster %d %d %d rect %d %d %d %d members %d score %.17g" % (tuple(c["index"]) + tuple(c["rect"]) + (c["member_count"], c["score"])) for c in clusters]
    assert len(clusters) >= 1 and res.stdout.strip().splitlines() == want
