"""The inputs of tests/test_gpu_second_trips.py, proven on the CPU with the headers alone (tests/second_trip_cases.py): every case
  crosses its cap          its shape, computed from the caps the compiled shims export, sends the loop it is about into a later trip
  depends on that trip     the header's answer changes when what only a later trip reads is blanked (tiles >= the score cap, pixels from
                           the pixel cap on, crop columns from one trip of a wave on): expected bytes that did not would prove nothing
and, on one reduced shape per family, the header equals its numpy restatement.  Each case prints its shape, the cap it crosses and how many
expected bytes depend on the later trips (pytest -s shows them)."""
import numpy as np
import pytest

import mesh_cases as mc
import normal_verify_cases as nvc
import pose_refine_cases as prc
import pose_refine_plane_cases as ppc
import pose_refine_staged_cases as psc
import pose_verify_cases as pvc
import scene_filter_cases as sfc
import second_trip_cases as stc
from linemod_pose_estimation_amd import POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE

WG = stc.WORKGROUP


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return stc.Hosts(tmp_path_factory.mktemp("second_trips"))


def differing(a, b):
    return int((np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8)).sum())


def report(case, shape, what, cap, size, nbytes):
    print("%-28s %-12s %-34s cap %8d, reaches %8d; %d expected bytes depend on the later trips" % (case, "%d x %d" % shape, what, cap, size, nbytes))


def test_the_caps_are_what_the_launches_need(hosts):
    c = hosts.caps
    assert c.vector == 8 and c.walk_lanes * c.vector >= 64 and c.tile_w * c.tile_h == WG          # a tile is one pixel per lane of a workgroup
    print("caps", vars(c))


SHAPES = {"filter/two_frames": (40, 6560), "filter/cut_rows_r7": (40, 4100), "filter/one_tile_over_mul_0": (32, 8200), "filter/one_tile_over_mul_16": (32, 8200),
          "normal_map_frames": (1053, 996), "normal_map_crops": [(129, 65), (520, 17), (129, 122)], "depth_crop": (261, 125), "wide": [(520, 6), (1025, 6), (1025, 3)]}


def test_the_shapes_are_those_of_the_caps_of_this_commit(hosts):
    """The builders follow the caps, so a raised cap does not make a case lose its later trip -- it makes the case larger.  This table holds
    the shapes at the caps this commit has: a changed cap shows here, with the names of the cases whose cost it changed."""
    caps = hosts.caps
    got = {"filter/" + c.name: c.shape for c in stc.filter_cases(caps)}
    got["normal_map_frames"] = stc.normal_frame_shape(caps)
    crops, first = stc.normal_crops(caps)
    got["normal_map_crops"] = [c.shape[::-1] for c in crops[first:]]
    got["depth_crop"] = stc.mesh_crop_case(caps)[3]
    got["wide"] = list(stc.wide_case(caps).sizes)
    moved = {k: (SHAPES[k], got[k]) for k in SHAPES if SHAPES[k] != got[k]}
    assert not moved and set(got) == set(SHAPES), "a cap moved (now %s) and these cases followed it, (was, is): %s -- see that each still takes a few seconds, then " \
                                                   "write the new shapes into SHAPES" % (vars(caps), moved)


def test_filter_frames_cross_both_caps_and_depend_on_the_later_trips(hosts):
    caps = hosts.caps
    cases = stc.filter_cases(caps)
    assert [c.name for c in cases] == ["two_frames", "cut_rows_r7", "one_tile_over_mul_0", "one_tile_over_mul_16"]
    for case in cases:
        W, H = case.shape
        tx, ty = stc.tiles_of(W, H, caps)
        want = case.want(hosts)
        assert case.tiles and tx * ty > caps.score_grid, "%s: %d tiles no longer pass the cap of %d workgroups" % (case.name, tx * ty, caps.score_grid)
        assert tx * ty <= caps.score_grid + 2 or case.name == "two_frames", (case.name, tx * ty)          # the smallest that crosses; two_frames also crosses the pixel cap
        if case.pixels:
            assert W * H > caps.apply_grid * WG, "%s: %d pixels no longer pass the cap of %d x %d" % (case.name, W * H, caps.apply_grid, WG)
            # the smallest that crosses: a workgroup's worth over the pixel cap, unless the tile cap asked for more rows
            assert W * H <= (caps.apply_grid + 2) * WG or tx * (ty - 1) <= caps.score_grid, (case.name, W * H)
        for f, frame in enumerate(case.frames):
            got, rec = want[f]
            late_tile = stc.tile_index(W, H, caps) >= caps.score_grid
            assert late_tile.any() and (frame[late_tile] != 0).any()
            removed = (frame != 0) & (got == 0)
            assert rec["n_removed"][0] > 0 and rec["n_scored"][0] > 0
            if case.mul == 1.0:                                                                           # at 0 and at 16 standard deviations the case is about the threshold
                assert removed[late_tile].any(), "%s frame %d: no outlier is removed in a tile >= %d" % (case.name, f, caps.score_grid)
            b_map, b_rec = stc.filter_by_header(hosts, stc.blank_later_tiles(frame, caps), case.cam, case.r, case.k, case.mul)
            assert b_rec.tobytes() != rec.tobytes() and (b_rec["sum_q"] != rec["sum_q"]).all(), (case.name, f)       # the sums carried over the tiles
            n = differing(b_map, got) + differing(b_rec, rec)
            assert (b_map != got)[late_tile].any() and n > 0, (case.name, f)
            report("filter/%s[%d]" % (case.name, f), (W, H), "tiles per frame", caps.score_grid, tx * ty, n)
            if case.pixels:
                first = caps.apply_grid * WG
                late = np.zeros(W * H, bool)
                late[first:] = True
                late = late.reshape(H, W)
                if case.mul == 1.0:
                    assert removed[late].any(), "%s frame %d: no outlier is removed from pixel %d on" % (case.name, f, first)
                p_map, p_rec = stc.filter_by_header(hosts, stc.blank_from_pixel(frame, first), case.cam, case.r, case.k, case.mul)
                n = differing(p_map, got) + differing(p_rec, rec)
                assert (p_map != got)[late].any() and n > 0, (case.name, f)
                report("filter/%s[%d]" % (case.name, f), (W, H), "pixels per frame", first, W * H, n)
    two = cases[0].want(hosts)
    assert two[0][1]["sum_q"][0] != two[1][1]["sum_q"][0] and two[0][1]["n_valid"][0] != two[1][1]["n_valid"][0] and two[0][1]["threshold"][0] != two[1][1]["threshold"][0]
    W, H = cases[0].shape
    assert W % caps.tile_w == caps.tile_w // 4 and stc.tiles_of(W, H, caps)[0] == 2                       # the right tile column is cut
    assert caps.score_grid < stc.tiles_of(W, H, caps)[0] * stc.tiles_of(W, H, caps)[1] < 2 * caps.score_grid        # some workgroups take two tiles, some one
    assert cases[1].shape[1] % caps.tile_h != 0 and cases[1].r == 7         # the cut last row of tiles, the largest halo


def test_filter_header_equals_the_numpy_restatement_on_a_reduced_cut_frame(hosts):
    for frame, r, k in stc.reduced_filter_frames(hosts.caps):
        cam = sfc.scene_camera(frame)
        got, rec = stc.filter_by_header(hosts, frame, cam, r, k, 1.0)
        want, wrec, _, _ = sfc.np_filter(frame, cam, r, k, 1.0)
        assert got.tobytes() == want.tobytes() and rec.tobytes() == sfc.record_array(wrec).tobytes(), (r, k)
        assert rec["n_removed"][0] > 0 and frame.shape[1] % hosts.caps.tile_w and frame.shape[0] % hosts.caps.tile_h


def test_normal_frames_cross_the_cap_with_valid_normals_beyond_it(hosts):
    caps = hosts.caps
    W, H = stc.normal_frame_shape(caps)
    first = caps.frame_map_grid * WG
    assert first < W * H <= first + WG, "the frame no longer has %d + 1 workgroups of pixels" % caps.frame_map_grid
    for f, frame in enumerate(stc.normal_frames(caps)):
        want = nvc.host_map(hosts.nv, frame)
        late = want.reshape(-1, 4)[first:]
        assert late[:, 3].any() and late[:, :3].any(), f
        blank = nvc.host_map(hosts.nv, stc.blank_from_pixel(frame, first))
        n = differing(blank, want)
        assert n > 0 and not blank.reshape(-1, 4)[first:].any()
        report("normal_map_frames[%d]" % f, (W, H), "pixels per frame", first, W * H, n)
    small = nvc.scene_image(70, 37, np.random.default_rng(33))
    assert np.array_equal(nvc.host_map(hosts.nv, small), nvc.np_normal_map(small))


def test_normal_crops_cross_the_cap_with_valid_normals_beyond_it(hosts):
    caps = hosts.caps
    crops, first_big = stc.normal_crops(caps)
    cap = caps.crop_map_grid * WG
    sizes = []
    for k, c in enumerate(crops):
        h, w = c.shape
        pitch = (w + caps.vector - 1) // caps.vector * caps.vector
        sizes.append(h * pitch)
        if k < first_big:
            assert h * pitch <= cap
            continue
        assert h * pitch > cap, "crop %d (%d x %d): %d elements no longer pass the cap of %d x %d" % (k, w, h, h * pitch, caps.crop_map_grid, WG)
        want = nvc.host_map(hosts.nv, c)
        blank = nvc.host_map(hosts.nv, stc.blank_crop_from_element(c, cap, caps))
        n = differing(blank, want)
        assert n > 0 and (want[..., 3] != blank[..., 3]).any(), "crop %d (%d x %d): no valid normal lies beyond element %d" % (k, w, h, cap)
        report("normal_map_crops[%d]" % k, (w, h), "elements h x pitch", cap, h * pitch, n)
    assert sizes[first_big] == sizes[first_big + 1] or max(sizes[first_big:first_big + 2]) <= cap + 2 * 520     # the 129 and the 520 wide crop cross it about alike
    assert sizes[-1] > 2 * cap
    assert np.array_equal(nvc.host_map(hosts.nv, crops[1]), nvc.np_normal_map(crops[1]))


def test_mesh_crop_crosses_the_copy_cap_and_its_last_rows_hold_the_object(hosts):
    caps = hosts.caps
    tri, cam, views, (w, h) = stc.mesh_crop_case(caps)
    _, depth, mask, rects = mc.expected(tri, cam, views)
    cap = caps.crop_copy_grid * WG
    vpr = (w + caps.vector - 1) // caps.vector
    assert rects[0, 2] > 0 and 4 * int(rects[0, 3]) * ((int(rects[0, 2]) + caps.vector - 1) // caps.vector) < cap and not rects[2].any()     # a small view, a view of nothing
    x, y, cw, ch = (int(v) for v in rects[1])
    assert (cw, ch) == (w, h) and w % caps.vector != 0, (rects[1], w, h)
    assert cap < h * vpr <= cap + vpr, "the box of %d x %d has %d vectors: not the first height above the cap of %d x %d" % (w, h, h * vpr, caps.crop_copy_grid, WG)
    crop = depth[1, y:y + h, x:x + w]
    pad = nvc.padded(crop, vpr * caps.vector).reshape(-1, caps.vector)
    assert pad[cap:].any() and (crop != 0).all()
    report("depth_crop", (w, h), "vectors h x pitch / %d" % caps.vector, cap, h * vpr, 2 * int((pad[cap:] != 0).sum()))
    # the host rasteriser against its own numpy restatement on the small view (mesh_cases.numpy_render)
    winner, z, _ = mc.numpy_render(tri, cam, views[0])
    assert np.array_equal(winner >= 0, mask[0] != 0)


def test_wide_crops_take_later_trips_and_every_answer_depends_on_them(hosts):
    caps = hosts.caps
    case = stc.wide_case(caps)
    dt = (POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE)
    trip = caps.walk_lanes * caps.vector
    vectors = [(w + caps.vector - 1) // caps.vector for w, _ in case.sizes]
    assert vectors[0] == caps.walk_lanes + 1 and vectors[1] == 2 * caps.walk_lanes + 1 and case.sizes[1][0] % caps.vector == 1, (case.sizes, caps.walk_lanes)
    assert all(3 <= h <= 6 for _, h in case.sizes) and case.scene.shape[1] >= case.sizes[1][0] + 40
    full = stc.wide_reference(hosts, case, case.crops, dt)
    blank = stc.wide_reference(hosts, case, [stc.blank_from_column(c, trip) for c in case.crops], dt)
    for i, (x, y, k) in enumerate(case.rows):
        w, h = case.sizes[k]
        meets_late = x + w > max(x + trip, 0) and x + trip < case.scene.shape[1]                          # columns >= trip meet the scene
        n = 0
        for name in ("diff", "ndiff"):
            a, b = getattr(full, name)[i], getattr(blank, name)[i]
            assert a[2] > b[2], (name, i)                                                                 # n_template counts the late columns wherever they lie
            n += differing(a, b)
        if meets_late:
            assert full.diff[i][1] > blank.diff[i][1] and full.diff[i][0] > blank.diff[i][0], i
            if h == 6:
                assert full.ndiff[i][4] > blank.ndiff[i][4] >= (1 if x >= 0 else 0), i                    # normals beyond column `trip`, and in front of it where that meets the scene
        for name in ("refine", "staged", "plane"):
            a, b = getattr(full, name)[i], getattr(blank, name)[i]
            assert a[0]["n_model"][0] > b[0]["n_model"][0] and a[0]["status"][0] not in (prc.NONE, prc.NO_OVERLAP), (name, i, a[0])
            if meets_late:
                assert a[0]["n_pairs_first"][0] > b[0]["n_pairs_first"][0] >= 0 and not np.array_equal(a[1], b[1]), (name, i)     # pairs found in columns >= trip
            n += differing(a[0], b[0]) + differing(a[1], b[1])
        assert full.verify[i]["n_model"][0] > blank.verify[i]["n_model"][0]
        n += differing(full.verify[i], blank.verify[i])
        report("wide[%d] at %d" % (k, x), (w, h), "vectors of a row", caps.walk_lanes, vectors[k], n)
    assert sum(int(p[2][:, 0].astype(bool).sum()) for p in full.plane) > 10                               # plane passes ran
    assert any(p[0]["reserved"][0] == 1 for p in full.staged) and any(v["status"][0] == pvc.OK for v in full.verify)
    assert not all(a[0].tobytes() == b[0].tobytes() for a, b in zip(full.plane, full.staged))
    # the headers against their restatements on a reduced crop of the same surface: the case's 3-row crop cut to 40 columns, inside the scene
    c = np.ascontiguousarray(case.crops[2][:, :40])
    rect = case.rects[2, :2]
    x, y = int(case.rows[6][0]), int(case.rows[6][1])
    normals = nvc.host_map(hosts.nv, case.scene, case.cam[0], case.cam[1])
    assert np.array_equal(normals, nvc.np_normal_map(case.scene, case.cam[0], case.cam[1]))
    rec, sums, plane = ppc.host_refine_plane(hosts.pose("prp"), case.P, case.stages, case.shifts, c, rect, case.scene, normals, x, y, POSE_REFINE_DTYPE)
    nrec, nsums, nplane, _ = ppc.np_refine_plane(case.P, case.stages, case.shifts, c, rect, case.scene, normals, x, y)
    assert rec.tobytes() == prc.record_array(nrec, POSE_REFINE_DTYPE).tobytes() and np.array_equal(sums, nsums) and np.array_equal(plane, nplane)
    srec, ssums = psc.host_refine_staged(hosts.pose("prs"), case.P, case.stages, c, rect, case.scene, x, y, POSE_REFINE_DTYPE)
    n2, s2, _ = psc.np_refine_staged(case.P, case.stages, c, rect, case.scene, x, y)
    assert srec.tobytes() == prc.record_array(n2, POSE_REFINE_DTYPE).tobytes() and np.array_equal(ssums, s2)
    vrec = pvc.host_verify(hosts.pose("pv"), case.PV, c, rect, case.scene, srec["R"][0].reshape(9), srec["t_mm"][0], POSE_VERIFY_DTYPE)
    assert vrec.tobytes() == pvc.record_array(pvc.np_verify(case.PV, c, rect, case.scene, srec["R"][0].reshape(9), srec["t_mm"][0]), POSE_VERIFY_DTYPE).tobytes()
