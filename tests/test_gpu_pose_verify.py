"""Pose verification on the device (csrc/lmx_verify.hip, k_pose_verify) against the CPU build of the header it shares with the host
(csrc/lmx_pose_verify.hpp through tests/cpp/pose_verify_host.cpp): every byte of every record.  Nothing here has a tolerance.  The
header itself is held against the numpy restatement, on the same cases, by tests/test_pose_verify_host.py."""
import numpy as np
import pytest

import pose_refine_cases as prc
import pose_verify_cases as pvc
from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE, DepthTemplates, _lib, keep_verified

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pvc.build_host(tmp_path_factory.mktemp("pvhost"))


@pytest.fixture(scope="module")
def constructed(host):
    """The single jobs, their crops in one object (and an empty one behind them), and what the header gives for each: computed once."""
    jobs = pvc.constructed_jobs()
    want = [pvc.host_verify(host, j.P, j.crop, j.rect_xy, j.scene, j.R, j.t, POSE_VERIFY_DTYPE) for j in jobs]
    t = DepthTemplates.from_crops([j.crop for j in jobs] + [np.zeros((0, 0), np.uint16)])
    rects = np.asarray([(j.rect_xy[0], j.rect_xy[1], j.crop.shape[1], j.crop.shape[0]) for j in jobs] + [(0, 0, 0, 0)], np.int32)
    yield t, jobs, want, rects
    t.close()


def one_match(template_id, class_index=0, x=0, y=0):
    m = np.zeros(1, MATCH_DTYPE)
    m["x"], m["y"], m["template_id"], m["class_index"], m["similarity"] = x, y, template_id, class_index, 90.0
    return m


def pose_records(R, t, n=1, status=prc.CONVERGED):
    p = np.zeros(n, POSE_REFINE_DTYPE)
    p["R"][:], p["t_mm"][:], p["status"] = R, t, status
    return p


def assert_records(got, want, what):
    for k in POSE_VERIFY_DTYPE.names:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    assert got.tobytes() == want.tobytes(), what


def test_constructed_jobs_equal_the_header(constructed):
    t, jobs, want, rects = constructed
    statuses = set()
    for k, j in enumerate(jobs):
        got = t.verify_poses(one_match(k), pose_records(j.R, j.t), j.scene, rects=rects, **pvc.verify_kwargs(j.P))
        assert_records(got, want[k], j.name)
        if j.expect == "all":
            assert got["rate"][0] == 1.0 and got["n_occupied"][0] == got["n_tested"][0] == got["n_model"][0] > 0, j.name
        elif j.expect == "none":
            assert got["n_occupied"][0] == 0 and got["status"][0] == pvc.OK, j.name
        elif j.expect == "outside":
            assert got["n_scene"][0] == 0 and got["status"][0] == pvc.OK and got["rate"][0] == 0.0, j.name
        elif j.expect in (pvc.EMPTY, pvc.GRID_TOO_LARGE):
            assert got["status"][0] == j.expect, j.name
        statuses.add(int(got["status"][0]))
    assert statuses == {pvc.OK, pvc.EMPTY, pvc.GRID_TOO_LARGE}
    # the match position plays no part: the pose places the model
    k = [j.name for j in jobs].index("identity_33x37")
    got = t.verify_poses(one_match(k, x=-500, y=77), pose_records(jobs[k].R, jobs[k].t), jobs[k].scene, rects=rects, **pvc.verify_kwargs(jobs[k].P))
    assert_records(got, want[k], "another match position")


def test_zeroed_records(constructed):
    t, jobs, want, rects = constructed
    k = [j.name for j in jobs].index("identity_33x37")
    j = jobs[k]
    m = np.concatenate([one_match(k), one_match(len(jobs)), one_match(k), one_match(len(jobs) + 9, class_index=5), one_match(k)])
    p = pose_records(j.R, j.t, 5)
    p["status"][2] = prc.NONE                       # nothing was refined for it
    p["R"][2] = float("nan")                        # and what its record holds is not looked at
    p["R"][3] = float("nan")                        # nor is another class's
    got = t.verify_poses(m, p, j.scene, class_index=0, rects=rects, **pvc.verify_kwargs(j.P))
    assert_records(got[0:1], want[k], "before")
    assert_records(got[4:5], want[k], "after")
    for i in (1, 2, 3):                             # an empty crop, LMX_POSE_NONE, a foreign class
        assert not got[i:i + 1].view(np.uint8).any(), i
    assert keep_verified(got, 0.3).tolist() == [True, False, False, False, True]


def test_seventy_jobs_over_three_frames_with_a_class_index(constructed, host):
    t, jobs, _, rects = constructed
    rng = np.random.RandomState(22)
    names = ("identity_33x37", "left_half_occluded", "turned_by_refine")
    scenes = [jobs[[j.name for j in jobs].index(n)].scene for n in names]
    wide = np.full((3, pvc.SCENE_H, pvc.SCENE_W + 9), 4242, np.uint16)          # what lies behind a row's end in memory is not the next row
    for f in range(3):
        wide[f, :, :pvc.SCENE_W] = scenes[f]
    frames = [wide[f, :, :pvc.SCENE_W] for f in range(3)]
    assert not frames[1].flags["C_CONTIGUOUS"]
    usable = [k for k, j in enumerate(jobs) if j.crop.shape[0] > 1 and not j.name.startswith("cap_")]
    offsets = [0, 30, 30, 70]                                                      # the middle frame has no matches
    m = np.zeros(70, MATCH_DTYPE)
    m["template_id"] = rng.choice(usable, 70)
    m["class_index"] = np.arange(70) % 3
    m["template_id"][m["class_index"] == 2] = len(jobs) + 7                        # another class's ids are not looked at
    p = np.zeros(70, POSE_REFINE_DTYPE)
    for i in range(70):                                                            # small turns about y and moves of a few mm around the jobs' own poses
        p["R"][i] = pvc.rotation_y(rng.uniform(-3.0, 3.0))
        p["t_mm"][i] = rng.uniform(-6.0, 6.0, 3) + (rng.uniform(-40.0, 40.0), 0.0, 0.0)
    p["status"] = prc.MAX_ITERATIONS
    P = pvc.make_params(voxel_mm=5.5, roi_margin=3)
    frame_of = np.repeat(np.arange(3), np.diff(offsets))
    for cls in (0, 1):
        got = t.verify_poses(m, p, frames, offsets, class_index=cls, rects=rects, **pvc.verify_kwargs(P))
        hit = 0
        for i in range(70):
            if m["class_index"][i] != cls:
                assert not got[i:i + 1].view(np.uint8).any(), i
                continue
            k = int(m["template_id"][i])
            want = pvc.host_verify(host, P, jobs[k].crop, rects[k, :2], np.ascontiguousarray(frames[frame_of[i]]), p["R"][i], p["t_mm"][i], POSE_VERIFY_DTYPE)
            assert_records(got[i:i + 1], want, (cls, i))
            hit += int(want["n_occupied"][0] > 0)
        assert hit >= 5
    with pytest.raises(_lib.LmxError) as e:                                        # without the filter the foreign ids are refused before any launch
        t.verify_poses(m, p, frames, offsets, rects=rects, **pvc.verify_kwargs(P))
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "match 2:" in str(e.value)


def test_resident_scene_and_poses_from_refine_poses(constructed, host):
    """refine_poses and verify_poses on one resident scene, the records of the first handed to the second as they come; the refinement's
    bytes are the same before and after: the new stage disturbs nothing it shares."""
    import torch
    t, jobs, _, rects = constructed
    names = [j.name for j in jobs]
    k = names.index("turned_by_refine")
    frames = [jobs[k].scene, jobs[names.index("identity_33x37")].scene]
    rx, ry = jobs[k].rect_xy
    m = np.concatenate([one_match(k, x=rx, y=ry), one_match(k, x=rx + 1, y=ry), one_match(k, x=rx, y=ry - 1)])
    offsets = [0, 1, 3]
    PR = prc.refine_kwargs(prc.make_params(prc.CAM, prc.CAM, max_dist_mm=40.0, max_iterations=40, min_pairs=16, search_radius=2))
    PV = pvc.make_params()
    poses = t.refine_poses(m, frames, offsets, rects=rects, **PR)
    assert (poses["iterations"] > 0).all()
    want = np.concatenate([pvc.host_verify(host, PV, jobs[k].crop, rects[k, :2], frames[f], poses["R"][i], poses["t_mm"][i], POSE_VERIFY_DTYPE)
                           for i, f in enumerate((0, 1, 1))])
    assert want["rate"][0] > 0.8                                                   # the turned object under the pose the device refined
    host_frames = t.verify_poses(m, poses, frames, offsets, rects=rects, **pvc.verify_kwargs(PV))
    assert_records(host_frames, want, "host frames")
    with pytest.raises(_lib.LmxError) as e:                                        # the call with host frames forgot any scene
        t.verify_poses(m, poses, None, offsets, rects=rects, **pvc.verify_kwargs(PV))
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "no scene" in str(e.value)
    t.upload_scene(frames)
    before = t.refine_poses(m, None, offsets, rects=rects, **PR)
    assert before.tobytes() == poses.tobytes()
    for _ in range(2):                                                             # the scene stays
        assert_records(t.verify_poses(m, before, None, offsets, rects=rects, **pvc.verify_kwargs(PV)), want, "upload_scene")
    assert t.refine_poses(m, None, offsets, rects=rects, **PR).tobytes() == before.tobytes()
    with pytest.raises(_lib.LmxError) as e:
        t.verify_poses(m, poses, None, [0, 1, 2, 3], rects=rects, **pvc.verify_kwargs(PV))
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "2 frames" in str(e.value)
    dev = [torch.from_numpy(f.view(np.int16).copy()).cuda() for f in frames]
    torch.cuda.synchronize()
    t.upload_scene_device(dev)
    assert_records(t.verify_poses(m, poses, None, offsets, rects=rects, **pvc.verify_kwargs(PV)), want, "upload_scene_device")
    swapped = t.verify_poses(m, poses, frames[::-1], offsets, rects=rects, **pvc.verify_kwargs(PV))   # the frame index reaches the kernel
    assert swapped.tobytes() != want.tobytes()


def test_refusals_happen_before_any_launch(constructed):
    t, jobs, _, rects = constructed
    j = jobs[0]
    kw = pvc.verify_kwargs(j.P)
    good = pose_records(j.R, j.t)
    t.set_profiling(True)
    try:
        t.verify_poses(one_match(0), good, j.scene, rects=rects, **kw)
        assert t.kernel_times()["k_pose_verify"][1] == 1
        nan = float("nan")
        for bad in (dict(voxel_mm=0.2), dict(voxel_mm=64.5), dict(voxel_mm=nan), dict(roi_margin=-1), dict(roi_margin=65), dict(scene_camera=(0.0, 400.0, 48.0, 40.0)),
                    dict(model_camera=(400.0, nan, 48.0, 40.0))):
            with pytest.raises(_lib.LmxError) as e:
                t.verify_poses(one_match(0), good, j.scene, rects=rects, **dict(kw, **bad))
            assert e.value.status == _lib.LMX_ERR_INVALID_ARG, bad
        two = np.concatenate([one_match(0), one_match(0)])
        for field, k, v in (("R", 3, nan), ("R", 8, 2.5), ("R", 0, float("inf")), ("t_mm", 0, -2.0 ** 20 - 1.0), ("t_mm", 2, nan)):
            p = pose_records(j.R, j.t, 2)
            p[field][1, k] = v
            with pytest.raises(_lib.LmxError) as e:
                t.verify_poses(two, p, j.scene, rects=rects, **kw)
            assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "match 1:" in str(e.value), (field, k, v)
        with pytest.raises(_lib.LmxError) as e:
            t.verify_poses(one_match(len(jobs) + 1), good, j.scene, rects=rects, **kw)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "template_id" in str(e.value)
        far = rects.copy()
        far[0, 1] = -(1 << 17) - 1
        with pytest.raises(_lib.LmxError) as e:
            t.verify_poses(one_match(0), good, j.scene, rects=far, **kw)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "rect" in str(e.value)
        assert t.kernel_times()["k_pose_verify"][1] == 1                          # nothing was launched for any of them
    finally:
        t.set_profiling(False)
