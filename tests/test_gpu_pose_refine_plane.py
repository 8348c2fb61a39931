"""Point-to-plane pose refinement on the device (csrc/lmx_verify.hip: the PLANE instantiations of pose_refine_body's kernels k_pose_refine,
k_pose_refine_clusters and k_rough_refine_clusters) against the CPU build of the header it shares with the host (refine_job_plane through
tests/cpp/pose_refine_plane_host.cpp): every byte of every record and every integer of both sum arrays of every pass.  Nothing here has a
tolerance.  The header itself is held against the numpy restatement, on the same cases, by tests/test_pose_refine_plane_host.py."""
import os
import subprocess

import numpy as np
import pytest

import pose_chain_cases as pcc
import pose_refine_cases as prc
import pose_refine_plane_cases as ppc
import pose_refine_staged_cases as psc
import pose_verify_cases as pvc
import test_gpu_pose_chain as tpc
import test_gpu_rough_pose as trp
from conftest import ROOT
from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, DepthTemplates, _lib, keep_verified

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ppc.build_host(tmp_path_factory.mktemp("prphost"))


@pytest.fixture(scope="module")
def constructed(host):
    """The plane jobs, one object per normal-map threshold holding its jobs' crops, and what the header gives for each: computed once."""
    jobs, scenes, normals = ppc.constructed_jobs(), ppc.scenes(), ppc.scene_normal_maps()
    want = [ppc.host_refine_plane(host, j.P, j.stages, j.shifts, j.crop, j.rect_xy, scenes[j.scene], normals[j.normals], j.x, j.y, POSE_REFINE_DTYPE) for j in jobs]
    objects = {}
    for suffix, threshold in ppc.DISTANCE_THRESHOLDS.items():
        mine = [k for k, j in enumerate(jobs) if j.normals == j.scene + suffix]
        t = DepthTemplates.from_crops([jobs[k].crop for k in mine])
        t.enable_normals(ppc.NORMAL_FX, ppc.NORMAL_FY, ppc.DIFF_T, threshold)
        rects = np.asarray([(jobs[k].rect_xy[0], jobs[k].rect_xy[1], jobs[k].crop.shape[1], jobs[k].crop.shape[0]) for k in mine], np.int32)
        objects[suffix] = (t, rects, {k: i for i, k in enumerate(mine)})
    where = lambda k: next((t, rects, index[k]) for t, rects, index in objects.values() if k in index)
    yield jobs, scenes, want, where
    for t, _, _ in objects.values():
        t.close()


def one_match(x, y, template_id, class_index=0):
    m = np.zeros(1, MATCH_DTYPE)
    m["x"], m["y"], m["template_id"], m["class_index"], m["similarity"] = x, y, template_id, class_index, 90.0
    return m


def assert_records(got, want, what):
    for k in POSE_REFINE_DTYPE.names:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    assert got.tobytes() == want.tobytes(), what


def test_constructed_jobs_equal_the_header(constructed):
    """The sums hook, refine_poses on a staged frame and refine_poses on the resident scene (the job's scene as frame 1 of 2)."""
    jobs, scenes, want, where = constructed
    steps = 0
    for k, j in enumerate(jobs):
        t, rects, i = where(k)
        kw = dict(rects=rects, **prc.refine_kwargs(j.P))
        t.set_refine_schedule(j.stages)
        t.set_refine_plane(j.shifts)
        assert t.get_refine_plane() == list(j.shifts)
        rec, sums, plane = t.debug_pose_refine_plane_sums(scenes[j.scene], one_match(j.x, j.y, i), **kw)
        assert np.array_equal(sums, want[k][1]), (j.name, np.nonzero((sums != want[k][1]).any(1))[0][:3])
        assert np.array_equal(plane, want[k][2]), (j.name, np.nonzero((plane != want[k][2]).any(1))[0][:3])
        assert_records(np.asarray([rec]), want[k][0], j.name)
        assert np.array_equal(t.debug_pose_refine_sums(scenes[j.scene], one_match(j.x, j.y, i), **kw)[1], want[k][1]), j.name   # the 17-sum hook under the setting
        assert_records(t.refine_poses(one_match(j.x, j.y, i), scenes[j.scene], **kw), want[k][0], (j.name, "staged frame"))
        other = scenes["plain" if j.scene != "plain" else "holes"]
        t.upload_scene([other, scenes[j.scene]])
        assert_records(t.refine_poses(one_match(j.x, j.y, i), None, [0, 0, 1], **kw), want[k][0], (j.name, "resident scene"))
        assert_records(t.refine_poses(one_match(j.x, j.y, i), None, [0, 0, 1], **kw), want[k][0], (j.name, "resident scene, normals kept"))
        steps += int(want[k][2][:, 0].astype(bool).sum())
        t.set_refine_plane(None)
        t.set_refine_schedule(None)
    assert steps > 40                                                                             # plane passes ran, on the device as on the host


def test_seventy_jobs_over_three_frames(constructed, host):
    """Many workgroups in one launch, each with its own frame's normals."""
    jobs, scenes, _, where = constructed
    names = [j.name for j in jobs]
    usable = [names.index(n) for n in ("crop_33x37_shift_8", "crop_8x8_shift_8", "holes", "radius_1_border", "radius_2_far_border")]
    t, rects, _ = where(usable[0])
    index = {k: where(k)[2] for k in usable}
    assert all(where(k)[0] is t for k in usable)
    normals = ppc.scene_normal_maps()
    rng = np.random.RandomState(23)
    frame_names = ("plain", "holes", "sparse")
    offsets = [0, 30, 30, 70]
    pick = rng.choice(usable, 70)
    m = np.zeros(70, MATCH_DTYPE)
    m["template_id"] = [index[k] for k in pick]
    m["x"], m["y"] = rects[m["template_id"], 0] + rng.randint(-3, 4, 70), rects[m["template_id"], 1] + rng.randint(-3, 4, 70)
    P = prc.make_params(prc.CAM, prc.CAM, max_dist_mm=12.0, max_iterations=3, min_pairs=6, search_radius=1)
    stages, shifts = psc.parse_schedule("2:2:12:1,1:2:12:1"), [8, 4]
    frame_of = np.repeat(np.arange(3), np.diff(offsets))
    t.set_refine_schedule(stages)
    t.set_refine_plane(shifts)
    try:
        got = t.refine_poses(m, [scenes[n] for n in frame_names], offsets, rects=rects, **prc.refine_kwargs(P))
        for i in range(70):
            f = frame_names[frame_of[i]]
            want, _, plane = ppc.host_refine_plane(host, P, stages, shifts, jobs[pick[i]].crop, rects[m["template_id"][i], :2], scenes[f], normals[f], m["x"][i], m["y"][i],
                                                   POSE_REFINE_DTYPE)
            assert_records(got[i:i + 1], want, i)
        assert (got["reserved"] == 1).sum() >= 40
        t.upload_scene([scenes[n] for n in frame_names])
        assert_records(t.refine_poses(m, None, offsets, rects=rects, **prc.refine_kwargs(P)), got, "resident")
    finally:
        t.set_refine_plane(None)
        t.set_refine_schedule(None)


def test_never_set_all_minus_one_and_cleared_give_the_same_bytes():
    jobs, scenes = prc.constructed_jobs(), prc.scenes()
    jobs = [j for j in jobs if j.name in ("crop_33x37", "holes", "radius_2_border", "off_left_top", "lost_later", "singular_row", "outside_right")]
    crops = [j.crop for j in jobs]
    rects = np.asarray([(j.rect_xy[0], j.rect_xy[1], j.crop.shape[1], j.crop.shape[0]) for j in jobs], np.int32)
    never, t = DepthTemplates.from_crops(crops), DepthTemplates.from_crops(crops)
    two = psc.parse_schedule("2:4:12:1,1:3:12:1")
    try:
        t.enable_normals(ppc.NORMAL_FX, ppc.NORMAL_FY)
        for schedule in (None, two):
            never.set_refine_schedule(schedule)
            t.set_refine_schedule(schedule)
            for k, j in enumerate(jobs):
                kw = dict(rects=rects, **prc.refine_kwargs(j.P))
                m = one_match(j.x, j.y, k)
                want = never.refine_poses(m, scenes[j.scene], **kw)
                want_sums = never.debug_pose_refine_sums(scenes[j.scene], m, **kw)[1]
                t.set_refine_plane([8, 4])
                other = t.refine_poses(m, scenes[j.scene], **kw)
                for setting in ([-1, -1, -1, -1], [-1], None):
                    t.set_refine_plane(setting)
                    assert_records(t.refine_poses(m, scenes[j.scene], **kw), want, (j.name, setting))
                    rec, sums, plane = t.debug_pose_refine_plane_sums(scenes[j.scene], m, **kw)
                    assert_records(np.asarray([rec]), want, (j.name, setting, "hook"))
                    assert np.array_equal(sums, want_sums) and not plane.any(), (j.name, setting)
                if j.name == "holes":
                    assert other.tobytes() != want.tobytes()                                       # the setting was in force in between
        # a shift beyond the schedule's stages governs nothing
        t.set_refine_schedule(None)
        t.set_refine_plane([-1, 8, 8, 8])
        j = jobs[1]
        kw = dict(rects=rects, **prc.refine_kwargs(j.P))
        never.set_refine_schedule(None)
        assert_records(t.refine_poses(one_match(j.x, j.y, 1), scenes[j.scene], **kw), never.refine_poses(one_match(j.x, j.y, 1), scenes[j.scene], **kw), "stage 0 alone")
    finally:
        never.close()
        t.close()


def test_pose_chain_under_the_setting_equals_the_host_composition(host):
    crops, rects = tpc.the_crops()
    t = DepthTemplates.from_crops(crops)
    try:
        t.enable_normals(ppc.NORMAL_FX, ppc.NORMAL_FY)
        scenes = [prc.make_scene(holes=0.25), pvc.paste(crops[0], (30, 20))]
        t.upload_scene(scenes)
        L = pcc.build_lists([(0, tpc.frame_matches(6, rects, 1), [[0, 1], [2], [3, 4, 5]]), (0, tpc.frame_matches(4, rects, 2, templates=(0, 3)), [[0, 2], [1, 3]])])
        plain = tpc.run_hook(t, L, rects)
        P = prc.make_params(prc.CAM, prc.CAM, max_dist_mm=12.0, max_iterations=6, min_pairs=3, search_radius=1)
        for stages, shifts in ((None, [8]), (psc.parse_schedule("2:4:12:1,1:3:12:1"), [4, -1]), (psc.parse_schedule("4:3:12:2,1:3:12:1"), [-1, 8])):
            t.set_refine_schedule(stages)
            t.set_refine_plane(shifts)
            want = pcc.host_staged(t, L, {0, 1}, 0, tpc.PR, tpc.PV, tpc.THRESH, rects)          # refine_poses and verify_poses on the leaders
            got = tpc.run_hook(t, L, rects)
            tpc.check_against_host(got, want, 5, 5, 0, shifts)
            assert got[2].tobytes() != plain[2].tobytes()
            for k, (lead, pose, _, _) in want.items():                                           # and the composition's refine step is the header's
                mm, f = L.matches[lead], 0 if lead < 6 else 1
                ref, _, _ = ppc.host_refine_plane(host, P, stages, shifts, crops[mm["template_id"]], rects[mm["template_id"], :2], scenes[f], ppc.scene_normals(scenes[f]),
                                                  mm["x"], mm["y"], POSE_REFINE_DTYPE)
                assert_records(pose, ref, ("slot", k, shifts))
        t.set_refine_plane(None)
        t.set_refine_schedule(None)
        assert tpc.run_hook(t, L, rects)[2].tobytes() == plain[2].tobytes()
    finally:
        t.close()


def test_rough_pose_chain_under_the_setting_equals_the_host_composition(host):
    """A coarse plane stage on the re-rendered crop: the lattice starts at the silhouette box inside the window the kernel walks."""
    tri, views, scene, L = trp.chain_setup()
    model = trp.model_of(views, tri=tri)
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    t2 = None
    stages = psc.parse_schedule("4:4:12:1,1:3:12:1", eps_rot_rad=1e-4, eps_trans_mm=1e-2)
    shifts = [8, 4]
    try:
        t.enable_normals(trp.CAM[0], trp.CAM[1])
        t.upload_scene(scene)
        t.set_refine_schedule(stages)
        t.set_refine_plane(shifts)
        hdr, rough, group, poses, checks, keep = trp.run_hook(t, model, L, trp.rpc.trace_min_of(10.0), room=2)
        n = len(L.clusters)
        assert hdr[0] == n == 9
        crops = [model.debug_crop(k) for k in range(n)]
        t2 = DepthTemplates.from_crops([c for c, _ in crops])
        t2.enable_normals(trp.CAM[0], trp.CAM[1])
        t2.upload_scene(scene)
        t2.set_refine_schedule(stages)
        t2.set_refine_plane(shifts)
        m = pcc.matches_of([(rough["x"][k], rough["y"][k], 90.0, k, 0) for k in range(n)])
        rects = np.asarray([r for _, r in crops], np.int32)
        offsets = [0, 4, 8, 9]
        want_p = t2.refine_poses(m, None, offsets, rects=rects, **trp.PR)
        want_c = t2.verify_poses(m, want_p, None, offsets, rects=rects, **trp.PV)
        assert_records(poses[:n], want_p, "rough chain")
        assert checks[:n].tobytes() == want_c.tobytes() and keep[:n].tolist() == keep_verified(want_c, trp.THRESH).astype(np.uint8).tolist()
        assert (want_p["reserved"] == 1).any()
        P = prc.make_params(trp.CAM, trp.CAM, max_dist_mm=12.0, eps_rot_rad=1e-4, eps_trans_mm=1e-2, max_iterations=64, min_pairs=3, search_radius=1)
        frame_of = np.repeat(np.arange(3), np.diff(offsets))
        planes = 0
        for k in range(n):
            f = frame_of[k]
            ref, _, pl = ppc.host_refine_plane(host, P, stages, shifts, crops[k][0], rects[k, :2], scene[f], ppc.scene_normals(scene[f], fx=trp.CAM[0], fy=trp.CAM[1]),
                                               m["x"][k], m["y"][k], POSE_REFINE_DTYPE)
            assert_records(poses[k:k + 1], ref, ("slot", k))
            planes += int(pl[:, 0].astype(bool).sum())
        assert planes > 0
    finally:
        model.close()
        t.close()
        if t2 is not None:
            t2.close()


def test_the_setter_next_to_device_work(constructed):
    jobs, scenes, want, where = constructed
    k = [j.name for j in jobs].index("holes")
    j = jobs[k]
    t, rects, i = where(k)
    kw = dict(rects=rects, **prc.refine_kwargs(j.P))
    t.set_refine_plane(j.shifts)
    try:
        for bad in ([21], [-2], [8] * 5):
            with pytest.raises(_lib.LmxError) as e:
                t.set_refine_plane(bad)
            assert e.value.status == _lib.LMX_ERR_INVALID_ARG and t.get_refine_plane() == list(j.shifts)
            assert_records(t.refine_poses(one_match(j.x, j.y, i), scenes[j.scene], **kw), want[k][0], "after a refusal")
        # an object that never enabled its normals refuses a shift >= 0 and goes on refining point-to-point
        bare = DepthTemplates.from_crops([j.crop])
        try:
            with pytest.raises(_lib.LmxError) as e:
                bare.set_refine_plane([8])
            assert "enable_normals" in str(e.value) and bare.get_refine_plane() == []
            one = np.asarray([rects[i]], np.int32)
            point = bare.refine_poses(one_match(j.x, j.y, 0), scenes[j.scene], **dict(kw, rects=one))
            assert point["iterations"][0] > 0 and point.tobytes() != want[k][0].tobytes()
        finally:
            bare.close()
    finally:
        t.set_refine_plane(None)


def test_cpp_caller_prints_what_python_computes(tmp_path):
    """tests/cpp/pose_refine_plane_main.cpp (a crop, the normals enabled, a schedule and the shifts set and read back, the matches refined under
    them and again without) against the same calls here."""
    c, r = prc.make_crop(33, 37, (30, 20))
    scene = prc.make_scene(holes=0.25)
    text, shifts = "4:3:12:1,1:3:12:1", [8, 4]
    places = [(30, 20), (28, 22), (-9, -11), (prc.SCENE_W, 10)]
    t = DepthTemplates.from_crops([c])
    rects = np.asarray([(r[0], r[1], 33, 37)], np.int32)
    m = np.concatenate([one_match(x, y, 0) for x, y in places])
    kw = dict(model_camera=prc.CAM, scene_camera=prc.CAM, rects=rects, max_iterations=5)

    def lines(what, poses):
        return ["%s match %d %d status %d stage %d iterations %d pairs %d %d rms %.17g %.17g R %s t %.17g %.17g %.17g"
                % (what, x, y, p["status"], p["reserved"], p["iterations"], p["n_pairs_first"], p["n_pairs_last"], p["rms_first_mm"], p["rms_last_mm"],
                   " ".join("%.17g" % v for v in p["R"].reshape(9)), p["t_mm"][0], p["t_mm"][1], p["t_mm"][2]) for (x, y), p in zip(places, poses)]

    t.enable_normals(prc.CAM[0], prc.CAM[1])
    t.set_refine_schedule(psc.parse_schedule(text))
    t.set_refine_plane(shifts)
    plane = t.refine_poses(m, scene, **kw)
    t.set_refine_plane(None)
    point = t.refine_poses(m, scene, **kw)
    t.close()
    assert plane.tobytes() != point.tobytes()
    want = ["plane " + " ".join("%d" % k for k in shifts)] + lines("plane", plane) + ["plane cleared 0"] + lines("point", point)
    exe = str(tmp_path / "pose_refine_plane_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_refine_plane_main.cpp"), "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    np.ascontiguousarray(c).tofile(tmp_path / "crop.u16")
    np.ascontiguousarray(scene).tofile(tmp_path / "scene.u16")
    res = subprocess.run([exe, str(tmp_path / "crop.u16"), "33", "37", str(r[0]), str(r[1]), str(tmp_path / "scene.u16"), str(prc.SCENE_W), str(prc.SCENE_H)]
                         + [repr(v) for v in prc.CAM] + [text, ",".join("%d" % k for k in shifts)] + ["%d,%d" % p for p in places], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want
