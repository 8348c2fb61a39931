"""Pose refinement on the device (csrc/lmx_verify.hip, k_pose_refine) against the CPU build of the header it shares with the host
(csrc/lmx_pose_refine.hpp through tests/cpp/pose_refine_host.cpp): every byte of every record and every integer sum of every pass
(lmx_debug_pose_refine_sums).  Nothing here has a tolerance.  The header itself is held against the numpy restatement, on the same
cases, by tests/test_pose_refine_host.py."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import pose_refine_cases as prc
from conftest import ROOT
from linemod_pose_estimation_amd import (MATCH_DTYPE, POSE_REFINE_DTYPE, DepthTemplates, Detector, NativeBank, _lib, cluster_leaders, cluster_matches_scored,
                                         compose_pose, depth_values, meshsynth as ms)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return prc.build_host(tmp_path_factory.mktemp("prhost"))


@pytest.fixture(scope="module")
def constructed(host):
    """The single jobs, their crops in one object, and what the header gives for each: computed once."""
    jobs, scenes = prc.constructed_jobs(), prc.scenes()
    want = [prc.host_refine(host, j.P, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE) for j in jobs]
    t = DepthTemplates.from_crops([j.crop for j in jobs] + [np.zeros((0, 0), np.uint16)])
    rects = np.asarray([(j.rect_xy[0], j.rect_xy[1], j.crop.shape[1], j.crop.shape[0]) for j in jobs] + [(0, 0, 0, 0)], np.int32)
    yield t, jobs, scenes, want, rects
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
    t, jobs, scenes, want, rects = constructed
    statuses = set()
    for k, j in enumerate(jobs):
        rec, sums = t.debug_pose_refine_sums(scenes[j.scene], one_match(j.x, j.y, k), rects=rects, **prc.refine_kwargs(j.P))
        assert np.array_equal(sums, want[k][1]), (j.name, np.nonzero((sums != want[k][1]).any(1))[0][:3])
        assert_records(np.asarray([rec]), want[k][0], j.name)
        got = t.refine_poses(one_match(j.x, j.y, k), scenes[j.scene], rects=rects, **prc.refine_kwargs(j.P))
        assert_records(got, want[k][0], j.name)
        if j.expect is not None:
            assert got["status"][0] == j.expect, j.name
        statuses.add(int(got["status"][0]))
    assert statuses == {prc.CONVERGED, prc.MAX_ITERATIONS, prc.NO_OVERLAP, prc.LOST}
    # an empty crop: a zeroed record, whatever the scene holds
    got = t.refine_poses(one_match(10, 10, len(jobs)), scenes["plain"], rects=rects, **prc.refine_kwargs(jobs[0].P))
    assert not got.view(np.uint8).any()


def test_seventy_jobs_over_three_frames_with_a_class_index(constructed, host):
    t, jobs, scenes, _, rects = constructed
    rng = np.random.RandomState(21)
    wide = np.full((3, prc.SCENE_H, prc.SCENE_W + 9), 4242, np.uint16)          # what lies behind a row's end in memory is not the next row
    for f, name in enumerate(("plain", "holes", "sparse")):
        wide[f, :, :prc.SCENE_W] = scenes[name]
    frames = [wide[f, :, :prc.SCENE_W] for f in range(3)]
    assert not frames[1].flags["C_CONTIGUOUS"]
    usable = [k for k, j in enumerate(jobs) if j.crop.shape[0] > 1]
    offsets = [0, 30, 30, 70]                                                      # the middle frame has no matches
    m = np.zeros(70, MATCH_DTYPE)
    m["template_id"] = rng.choice(usable, 70)
    m["x"], m["y"] = rng.randint(-12, prc.SCENE_W - 8, 70), rng.randint(-10, prc.SCENE_H - 6, 70)
    m["class_index"] = np.arange(70) % 3
    m["template_id"][m["class_index"] == 2] = len(jobs) + 7                        # another class's ids are not looked at
    P = prc.make_params(prc.CAM, prc.CAM, max_dist_mm=12.0, max_iterations=5, min_pairs=6, search_radius=1)
    frame_of = np.repeat(np.arange(3), np.diff(offsets))
    for cls in (0, 1):
        got = t.refine_poses(m, frames, offsets, class_index=cls, rects=rects, **prc.refine_kwargs(P))
        ran = 0
        for i in range(70):
            if m["class_index"][i] != cls:
                assert not got[i:i + 1].view(np.uint8).any(), i
                continue
            k = int(m["template_id"][i])
            want, _ = prc.host_refine(host, P, jobs[k].crop, rects[k, :2], np.ascontiguousarray(frames[frame_of[i]]), m["x"][i], m["y"][i], POSE_REFINE_DTYPE)
            assert_records(got[i:i + 1], want, (cls, i))
            ran += int(want["iterations"][0] > 0)
        assert ran >= 10
    with pytest.raises(_lib.LmxError) as e:                                        # without the filter the foreign ids are refused before any launch
        t.refine_poses(m, frames, offsets, rects=rects, **prc.refine_kwargs(P))
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "match 2:" in str(e.value)


def test_resident_scene_equals_host_frames(constructed):
    import torch
    t, jobs, scenes, _, rects = constructed
    frames = [scenes["holes"], scenes["plain"]]
    k = [j.name for j in jobs].index("crop_33x37")
    m = np.concatenate([one_match(30, 20, k), one_match(28, 22, k), one_match(-9, -11, k)])
    offsets = [0, 1, 3]
    P = prc.refine_kwargs(jobs[k].P)
    want = t.refine_poses(m, frames, offsets, rects=rects, **P)
    assert (want["iterations"] > 0).all() and want[0].tobytes() != want[1].tobytes()
    with pytest.raises(_lib.LmxError) as e:                                        # the call with host frames forgot any scene
        t.refine_poses(m, None, offsets, rects=rects, **P)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "no scene" in str(e.value)
    t.upload_scene(frames)
    for _ in range(2):                                                             # the scene stays
        assert_records(t.refine_poses(m, None, offsets, rects=rects, **P), want, "upload_scene")
    with pytest.raises(_lib.LmxError) as e:
        t.refine_poses(m, None, [0, 1, 2, 3], rects=rects, **P)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "2 frames" in str(e.value)
    dev = [torch.from_numpy(f.view(np.int16).copy()).cuda() for f in frames]
    torch.cuda.synchronize()
    t.upload_scene_device(dev)
    assert_records(t.refine_poses(m, None, offsets, rects=rects, **P), want, "upload_scene_device")
    swapped = t.refine_poses(m, frames[::-1], offsets, rects=rects, **P)          # the frame index reaches the kernel
    assert swapped.tobytes() != want.tobytes()


def test_refusals_on_the_device(constructed):
    t, jobs, scenes, _, rects = constructed
    P = prc.refine_kwargs(jobs[0].P)
    for bad in (dict(max_iterations=65), dict(min_pairs=2), dict(search_radius=3), dict(max_dist_mm=0.0), dict(scene_camera=(0.0, 400.0, 48.0, 40.0)),
                dict(model_camera=(400.0, float("nan"), 48.0, 40.0))):
        with pytest.raises(_lib.LmxError) as e:
            t.refine_poses(one_match(30, 20, 0), scenes["plain"], rects=rects, **dict(P, **bad))
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG, bad
    with pytest.raises(_lib.LmxError) as e:
        t.refine_poses(one_match(30, 20, len(jobs) + 1), scenes["plain"], rects=rects, **P)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "template_id" in str(e.value)
    far = rects.copy()
    far[0, 1] = -(1 << 17) - 1
    with pytest.raises(_lib.LmxError) as e:
        t.refine_poses(one_match(30, 20, 0), scenes["plain"], rects=far, **P)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "rect" in str(e.value)


def test_ground_truth_on_the_device(host):
    g = prc.ground_truth_case()
    t = DepthTemplates.from_crops([g["crop"]])
    rects = np.asarray([g["rect"]], np.int32)
    bx, by = g["rect_b"][:2]
    errs = {}
    for it in (0, 20):
        P = prc.make_params(prc.GT_CAM, prc.GT_CAM, max_iterations=it)
        want, want_sums = prc.host_refine(host, P, g["crop"], g["rect"][:2], g["scene"], bx, by, POSE_REFINE_DTYPE)
        rec, sums = t.debug_pose_refine_sums(g["scene"], one_match(bx, by, 0), rects=rects, **prc.refine_kwargs(P))
        assert np.array_equal(sums, want_sums)
        assert_records(np.asarray([rec]), want, ("ground truth", it))
        R_obj, t_obj = compose_pose((g["R_a"], g["distance"]), rec)
        errs[it] = prc.pose_errors(R_obj, t_obj, g["R_b"], g["T_b_m"])
    assert rec["status"] in (prc.CONVERGED, prc.MAX_ITERATIONS) and rec["rms_last_mm"] < rec["rms_first_mm"]
    assert errs[20][0] < errs[0][0] and errs[20][1] < errs[0][1], errs
    t.close()


# ---- end to end, from Python and from C++ --------------------------------------------------------------------------------------------------

F = ms.ENSENSO["fx"]
W, H = 320, 240
THRESHOLD = 75.0


def test_cpp_caller_prints_what_python_computes(tmp_path):
    """tests/cpp/pose_refine_main.cpp (train from a mesh, match, cluster, refine each cluster's leader, compose) against the same chain here."""
    chip, cpu = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary")
    views = ms.view_grid()[:204]
    b = ms.empty_bank()
    nb = NativeBank.create(b.T, b.modalities)
    nb.train_mesh(chip, views, W, H, F / 2, F / 2)
    sc = nb.last_side_car
    sources, _ = ms.make_scene(chip, views, width=W, height=H, seed=11, n_instances=2, fx=F / 2, fy=F / 2, other_tri=cpu, n_other=1, margin=44)
    det = Detector(nb, W, H)
    matches = det.match(sources, THRESHOLD)
    det.close()
    template_views = list(zip(sc["R"], sc["T"][:, 2]))
    t = DepthTemplates.from_mesh(chip, template_views, W, H, F / 2, F / 2)
    clusters, members = cluster_matches_scored(matches, depth_values(t.diff(sources[1], matches)), sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
    lead = cluster_leaders(clusters, members, matches)
    assert len(lead) >= 1
    cam = (F / 2, F / 2, W / 2.0, H / 2.0)
    poses = t.refine_poses(matches[lead], sources[1], model_camera=cam, scene_camera=cam)
    assert (poses["status"] != 0).all() and (poses["iterations"] > 0).any() and (poses["rms_last_mm"][poses["iterations"] > 0] > 0).all()
    want = ["templates %d matches %d clusters %d" % (len(sc["rects"]), len(matches), len(clusters))]
    for k, (i, p) in enumerate(zip(lead, poses)):
        m = matches[i]
        R_obj, t_obj = compose_pose(template_views[int(m["template_id"])], p)
        want.append("cluster %d leader %d %d %d status %d iterations %d pairs %d %d rms %.17g %.17g R %s t %.17g %.17g %.17g"
                    % (k, m["x"], m["y"], m["template_id"], p["status"], p["iterations"], p["n_pairs_first"], p["n_pairs_last"], p["rms_first_mm"], p["rms_last_mm"],
                       " ".join("%.17g" % v for v in R_obj.reshape(9)), t_obj[0], t_obj[1], t_obj[2]))
    t.close()
    exe = str(tmp_path / "pose_refine_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_refine_main.cpp"),
                           "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    np.ascontiguousarray(chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(views).tofile(tmp_path / "views.f64")
    np.ascontiguousarray(sources[0]).tofile(tmp_path / "bgr.u8")
    np.ascontiguousarray(sources[1]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(W), str(H), repr(F / 2), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(THRESHOLD)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want
