"""Every size-capped loop of the pose-side kernels on a shape that sends it into a later trip (tests/second_trip_cases.py; proven to cross
the cap and to matter by tests/test_second_trip_cases_host.py), against the CPU builds of the shared headers, byte for byte:
  k_scene_filter_score    tiles blockIdx.x, + gridDim.x: the LDS points refilled behind a barrier, the per-lane sums carried over the tiles
  k_scene_filter_apply    pixels beyond one pass of the grid
  k_normal_map_frames / k_normal_map_crops / k_depth_crop    the same grid stride over pixels, elements, vectors
  diff_walk, crop_pixels  a lane's second and third vector of a crop row, in every kernel that ends in them
Nothing here has a tolerance."""
import numpy as np
import pytest

import depth_verify_cases as dvc
import mesh_cases as mc
import normal_verify_cases as nvc
import pose_chain_cases as pcc
import pose_refine_cases as prc
import pose_verify_cases as pvc
import scene_filter_cases as sfc
import second_trip_cases as stc
from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE, DepthTemplates, cluster_leaders, keep_verified
from test_gpu_normal_verify import d_rows, n_rows, strided

pytestmark = pytest.mark.gpu

WG = stc.WORKGROUP
CANARY = 0x5a
THRESH = 0.3


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return stc.Hosts(tmp_path_factory.mktemp("second_trips_gpu"))


@pytest.fixture(scope="module")
def plain():
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    yield t
    t.close()


# ---- the scene filter ------------------------------------------------------------------------------------------------------------------------------

def filter_case(hosts, name):
    return next(c for c in stc.filter_cases(hosts.caps) if c.name == name)


def run_filter_case(plain, hosts, case):
    """The upload through the setting and the hook against the header: the map and the whole record of every frame (what
    test_gpu_scene_filter.check_frames asserts, against the reference the CPU test has proven and this module computes once)."""
    plain.set_scene_filter(case.r, case.k, case.mul, camera=case.cam)
    plain.upload_scene(case.frames)
    got = [plain.debug_scene_filtered(f) for f in range(len(case.frames))]
    want = case.want(hosts)
    for f, ((filtered, info), (wmap, wrec)) in enumerate(zip(got, want)):
        bad = np.argwhere(filtered != wmap)
        assert len(bad) == 0, (case.name, f, "first differing pixel (row, column)", bad[0], "tile", int(stc.tile_index(*case.shape, hosts.caps)[tuple(bad[0])]))
        assert sfc.record_array(info).tobytes() == wrec.tobytes(), (case.name, f, info, wrec)
    return got


def test_filter_two_frames_beyond_both_caps(plain, hosts):
    caps = hosts.caps
    case = filter_case(hosts, "two_frames")
    W, H = case.shape
    assert 2 * (H // caps.tile_h) > caps.score_grid and W * H > caps.apply_grid * WG
    got = run_filter_case(plain, hosts, case)
    assert got[0][1]["sum_q"] != got[1][1]["sum_q"] and got[0][1]["threshold"] != got[1][1]["threshold"] and got[0][1]["n_valid"] != got[1][1]["n_valid"]
    late_tile = stc.tile_index(W, H, caps) >= caps.score_grid
    for f, frame in enumerate(case.frames):
        removed = (frame != 0) & (got[f][0] == 0)
        assert removed[late_tile].any() and removed.reshape(-1)[caps.apply_grid * WG:].any() and got[f][1]["n_removed"] > 0, f


def test_filter_cut_rows_with_the_largest_halo(plain, hosts):
    case = filter_case(hosts, "cut_rows_r7")
    assert case.shape[1] % hosts.caps.tile_h != 0 and case.r == 7
    got = run_filter_case(plain, hosts, case)
    assert got[0][1]["n_removed"] > 0 and got[0][1]["n_scored"] > 0


@pytest.mark.parametrize("mul", [0.0, 16.0])
def test_filter_one_tile_over_the_cap(plain, hosts, mul):
    case = filter_case(hosts, "one_tile_over_mul_%g" % mul)
    tx, ty = stc.tiles_of(*case.shape, hosts.caps)
    assert tx * ty == hosts.caps.score_grid + 1
    got = run_filter_case(plain, hosts, case)
    assert got[0][1]["n_scored"] > 0 and (got[0][1]["n_removed"] > got[0][1]["n_scored"] // 10) == (mul == 0.0)     # above the mean: about a fifth; 16 deviations out: next to none


# ---- the normal maps -------------------------------------------------------------------------------------------------------------------------------

def test_scene_normal_map_beyond_one_pass_of_the_grid(hosts):
    caps = hosts.caps
    frames = stc.normal_frames(caps)
    first = caps.frame_map_grid * WG
    assert frames[0].size > first
    t = DepthTemplates.from_crops([np.ones((3, 3), np.uint16)])
    try:
        t.enable_normals(nvc.FX, nvc.FY)
        views = strided(frames)
        assert not views[0].flags["C_CONTIGUOUS"]
        t.upload_scene(views)
        for f, img in enumerate(frames):
            got, want = t.debug_scene_normals(f), nvc.host_map(hosts.nv, img)
            bad = np.nonzero((got != want).any(-1).reshape(-1))[0]
            assert len(bad) == 0, (f, "first differing pixel", int(bad[0]), "of", img.size)
            assert want.reshape(-1, 4)[first:, 3].any(), f
    finally:
        t.close()


def test_crop_normal_maps_beyond_one_pass_of_the_grid(hosts):
    caps = hosts.caps
    crops, first_big = stc.normal_crops(caps)
    t = DepthTemplates.from_crops(crops)
    try:
        t.enable_normals(nvc.FX, nvc.FY)
        for k, c in enumerate(crops):
            got, want = t.normals(k), nvc.host_map(hosts.nv, c)
            bad = np.argwhere((got != want).any(-1))
            assert got.shape == c.shape + (4,) and len(bad) == 0, (k, c.shape, "first differing pixel (row, column)", bad[:1])
            assert np.array_equal(t.crop(k), c)
            if k >= first_big:
                assert c.shape[0] * ((c.shape[1] + caps.vector - 1) // caps.vector * caps.vector) > caps.crop_map_grid * WG and want[-1, :, 3].any(), k
    finally:
        t.close()


# ---- from_mesh's crop copy ----------------------------------------------------------------------------------------------------------------------------

def test_from_mesh_crop_copy_beyond_one_pass_of_the_grid(hosts):
    caps = hosts.caps
    tri, cam, views, (w, h) = stc.mesh_crop_case(caps)
    _, depth, _, rects = mc.expected(tri, cam, views)
    assert h * ((w + caps.vector - 1) // caps.vector) > caps.crop_copy_grid * WG
    t = DepthTemplates.from_mesh(tri, views, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    try:
        assert len(t) == 3
        padded = 0
        for i in range(3):
            x, y, cw, ch = (int(v) for v in rects[i])
            assert t.rect(i) == (x, y, cw, ch), i
            got = t.crop(i)
            bad = np.argwhere(got != depth[i, y:y + ch, x:x + cw])
            assert got.shape == (ch, cw) and len(bad) == 0, (i, "first differing pixel (row, column)", bad[:1])
            padded += ch * ((cw + 7) // 8 * 8) * 2
        assert t.rect(1)[2:] == (w, h) and t.rect(2) == (0, 0, 0, 0)
        assert padded <= t.device_bytes <= padded + 24 * 3                             # rows padded to 16 bytes, 24 bytes of table per template
        # the padding rule: what lies behind a row's end in the stored crop is zeros -- a scene of ones counts the object's pixels alone
        x, y = t.rect(1)[:2]
        d = t.diff(np.ones((cam["height"], cam["width"]), np.uint16), dvc.match_records(MATCH_DTYPE, [(x, y, 1)]))
        crop = depth[1, y:y + h, x:x + w].astype(np.int64)
        assert (int(d["sum_abs_mm"][0]), int(d["n_valid"][0]), int(d["n_template"][0])) == (int((crop - 1).sum()), w * h, w * h)
    finally:
        t.close()


# ---- crops wider than one trip of a wave along a row -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide(hosts):
    case = stc.wide_case(hosts.caps)
    want = stc.wide_reference(hosts, case, case.crops, (POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE))
    t = DepthTemplates.from_crops(case.crops)
    t.enable_normals(case.cam[0], case.cam[1])
    m = dvc.match_records(MATCH_DTYPE, case.rows)
    yield SimpleCase(case, want, t, m)
    t.close()


class SimpleCase:
    def __init__(self, case, want, t, m):
        self.case, self.want, self.t, self.m = case, want, t, m
        self.kw = dict(rects=case.rects, **prc.refine_kwargs(case.P))


def assert_records(got, want, what):
    for k in got.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    assert got.tobytes() == want.tobytes(), what


def test_wide_crops_depth_and_normal_terms(wide):
    c, t = wide.case, wide.t
    assert c.sizes[0][0] > c.trip and c.sizes[1][0] > 2 * c.trip
    for k, crop in enumerate(c.crops):
        assert np.array_equal(t.crop(k), crop), k
    d = t.diff(c.scene, wide.m)
    assert np.array_equal(d_rows(d), wide.want.diff), [(c.rows[i].tolist(), d_rows(d)[i].tolist(), wide.want.diff[i].tolist()) for i in np.nonzero((d_rows(d) != wide.want.diff).any(1))[0][:3]]
    dd, nd = t.normal_diff(c.scene, wide.m)
    got = np.concatenate([d_rows(dd), n_rows(nd)], 1)
    assert np.array_equal(got, wide.want.ndiff), [(c.rows[i].tolist(), got[i].tolist(), wide.want.ndiff[i].tolist()) for i in np.nonzero((got != wide.want.ndiff).any(1))[0][:3]]
    assert dd.tobytes() == d.tobytes() and (wide.want.ndiff[:, 4] > 0).sum() >= 5


def test_wide_crops_refined_without_a_schedule_and_verified(wide, hosts):
    c, t = wide.case, wide.t
    got = t.refine_poses(wide.m, c.scene, **wide.kw)
    for i in range(len(wide.m)):
        assert_records(got[i:i + 1], wide.want.refine[i][0], ("refine", c.rows[i].tolist()))
        rec, sums = t.debug_pose_refine_sums(c.scene, wide.m[i:i + 1], **wide.kw)
        assert np.array_equal(sums, wide.want.refine[i][1]), ("sums", c.rows[i].tolist(), np.nonzero((sums != wide.want.refine[i][1]).any(1))[0][:3])
        assert_records(np.asarray([rec]), wide.want.refine[i][0], ("hook", i))
    checks = t.verify_poses(wide.m, got, c.scene, rects=c.rects, **pvc.verify_kwargs(c.PV))
    for i in range(len(wide.m)):
        assert_records(checks[i:i + 1], wide.want.verify[i], ("verify", c.rows[i].tolist()))
    assert (checks["status"] == pvc.OK).any() and (got["iterations"] > 0).all()
    t.upload_scene(c.scene)                                                        # and on the resident scene
    assert_records(t.refine_poses(wide.m, None, [0, len(wide.m)], **wide.kw), got, "resident")
    assert_records(t.verify_poses(wide.m, got, None, [0, len(wide.m)], rects=c.rects, **pvc.verify_kwargs(c.PV)), checks, "resident")


def test_wide_crops_refined_under_a_schedule_and_with_plane_stages(wide):
    c, t = wide.case, wide.t
    t.set_refine_schedule(c.stages)
    try:
        got = t.refine_poses(wide.m, c.scene, **wide.kw)
        for i in range(len(wide.m)):
            assert_records(got[i:i + 1], wide.want.staged[i][0], ("staged", c.rows[i].tolist()))
            assert np.array_equal(t.debug_pose_refine_sums(c.scene, wide.m[i:i + 1], **wide.kw)[1], wide.want.staged[i][1]), ("staged sums", i)
        t.set_refine_plane(c.shifts)
        got = t.refine_poses(wide.m, c.scene, **wide.kw)
        planes = 0
        for i in range(len(wide.m)):
            wrec, wsums, wplane = wide.want.plane[i]
            assert_records(got[i:i + 1], wrec, ("plane", c.rows[i].tolist()))
            rec, sums, plane = t.debug_pose_refine_plane_sums(c.scene, wide.m[i:i + 1], **wide.kw)
            assert np.array_equal(sums, wsums), ("plane: the 17 sums", i, np.nonzero((sums != wsums).any(1))[0][:3])
            assert np.array_equal(plane, wplane), ("plane: the 29 sums", i, np.nonzero((plane != wplane).any(1))[0][:3])
            assert np.array_equal(t.debug_pose_refine_sums(c.scene, wide.m[i:i + 1], **wide.kw)[1], wsums), ("plane: the 17-sum hook", i)
            assert_records(np.asarray([rec]), wrec, ("plane hook", i))
            planes += int(wplane[:, 0].astype(bool).sum())
        assert planes > 10
    finally:
        t.set_refine_plane(None)
        t.set_refine_schedule(None)


def test_a_wide_crop_through_the_cluster_kernels(wide):
    """debug_pose_chain: k_pose_refine_clusters and k_pose_verify_clusters end in the same crop_pixels.  Two clusters of the 1025 x 6 crop's
    three placements; the records are the headers' for each cluster's leader."""
    c, t = wide.case, wide.t
    mine = [i for i, row in enumerate(c.rows) if row[2] == c.chain_crop]
    m = wide.m[mine].copy()
    m["similarity"] = [70.0, 90.0, 80.0]
    L = pcc.build_lists([(0, m, [[0, 1], [2]])])
    lead = cluster_leaders(L.clusters, L.members, L.matches)
    assert [int(v) for v in lead] == [1, 2]
    t.upload_scene(c.scene)
    kw = dict(prc.refine_kwargs(c.P), **{k: v for k, v in pvc.verify_kwargs(c.PV).items() if k not in prc.refine_kwargs(c.P)})
    hdr, leaders, poses, checks, keep = t.debug_pose_chain(L.header, L.frame_info, L.matches, L.clusters, L.members, THRESH, fill=CANARY, class_index=0, rects=c.rects, **kw)
    want_p = np.concatenate([wide.want.refine[mine[int(i)]][0] for i in lead])
    want_c = np.concatenate([wide.want.verify[mine[int(i)]] for i in lead])
    want_k = keep_verified(want_c, THRESH)
    assert [int(v) for v in leaders] == [int(v) for v in lead]
    assert_records(poses, want_p, "chain poses")
    assert_records(checks, want_c, "chain checks")
    assert keep.tolist() == want_k.astype(np.uint8).tolist()
    assert hdr.tolist() == [2, 0, int((want_p["status"] != prc.NONE).sum()), int((want_c["status"] == pvc.OK).sum()), int(want_k.sum()), 0, 0, 0]
