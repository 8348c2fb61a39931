"""Pose refinement under a schedule on the device (csrc/lmx_verify.hip: pose_refine_body's stage loop and lattice walk, shared by
k_pose_refine, k_pose_refine_clusters and k_rough_refine_clusters) against the CPU build of the header it shares with the host
(refine_job_staged through tests/cpp/pose_refine_staged_host.cpp): every byte of every record and every integer sum of every pass.
Nothing here has a tolerance.  The header itself is held against the numpy restatement, on the same cases, by
tests/test_pose_refine_staged_host.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import pose_chain_cases as pcc
import pose_refine_cases as prc
import pose_refine_staged_cases as psc
import pose_verify_cases as pvc
import test_gpu_pose_chain as tpc
import test_gpu_rough_pose as trp
from conftest import ROOT
from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, DepthTemplates, _lib, compose_pose, keep_verified

pytestmark = pytest.mark.gpu

TWO = psc.parse_schedule("2:4:12:1,1:3:12:1")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return psc.build_host(tmp_path_factory.mktemp("prshost"))


@pytest.fixture(scope="module")
def constructed(host):
    """The staged jobs, their distinct crops in one object, and what the header gives for each: computed once."""
    jobs, scenes = psc.constructed_jobs(), psc.scenes()
    want = [psc.host_refine_staged(host, j.P, j.stages, j.crop, j.rect_xy, scenes[j.scene], j.x, j.y, POSE_REFINE_DTYPE) for j in jobs]
    crops, index = [], []
    for j in jobs:
        at = [k for k, c in enumerate(crops) if c is j.crop]
        if not at:
            crops.append(j.crop)
        index.append(at[0] if at else len(crops) - 1)
    rects = np.zeros((len(crops), 4), np.int32)
    for j, k in zip(jobs, index):
        rects[k] = (j.rect_xy[0], j.rect_xy[1], j.crop.shape[1], j.crop.shape[0])
    t = DepthTemplates.from_crops(crops)
    yield t, jobs, scenes, want, rects, index
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
    t, jobs, scenes, want, rects, index = constructed
    seen = set()
    for k, j in enumerate(jobs):
        t.set_refine_schedule(j.stages)
        rec, sums = t.debug_pose_refine_sums(scenes[j.scene], one_match(j.x, j.y, index[k]), rects=rects, **prc.refine_kwargs(j.P))
        assert np.array_equal(sums, want[k][1]), (j.name, np.nonzero((sums != want[k][1]).any(1))[0][:3])
        assert_records(np.asarray([rec]), want[k][0], j.name)
        got = t.refine_poses(one_match(j.x, j.y, index[k]), scenes[j.scene], rects=rects, **prc.refine_kwargs(j.P))
        assert_records(got, want[k][0], j.name)
        for name, v in (j.expect or {}).items():
            assert got[name][0] == v, (j.name, name)
        seen.add((int(got["status"][0]), int(got["reserved"][0])))
    t.set_refine_schedule(None)
    assert {(prc.LOST, 0), (prc.LOST, 1), (prc.CONVERGED, 1), (prc.MAX_ITERATIONS, 1)} <= seen and any(s == 3 for _, s in seen), seen


def test_ground_truth_on_the_device(host):
    g = prc.ground_truth_case()
    t = DepthTemplates.from_crops([g["crop"]])
    rects = np.asarray([g["rect"]], np.int32)
    bx, by = g["rect_b"][:2]
    P = prc.make_params(prc.GT_CAM, prc.GT_CAM)
    try:
        placed = t.refine_poses(one_match(bx, by, 0), g["scene"], rects=rects, **prc.refine_kwargs(dict(P, max_iterations=0)))[0]
        e0 = prc.pose_errors(*compose_pose((g["R_a"], g["distance"]), placed), g["R_b"], g["T_b_m"])
        for text in psc.GT_SCHEDULES:
            stages = psc.parse_schedule(text)
            t.set_refine_schedule(stages)
            want, want_sums = psc.host_refine_staged(host, P, stages, g["crop"], g["rect"][:2], g["scene"], bx, by, POSE_REFINE_DTYPE)
            rec, sums = t.debug_pose_refine_sums(g["scene"], one_match(bx, by, 0), rects=rects, **prc.refine_kwargs(P))
            assert np.array_equal(sums, want_sums), text
            assert_records(np.asarray([rec]), want, text)
            err = prc.pose_errors(*compose_pose((g["R_a"], g["distance"]), rec), g["R_b"], g["T_b_m"])
            print("%s: status %d in stage %d after %d iterations, rotation error %.4f deg, translation error %.4f mm (placement %.4f, %.4f)"
                  % (text, rec["status"], rec["reserved"], rec["iterations"], err[0], err[1], e0[0], e0[1]))
            assert rec["status"] in (prc.CONVERGED, prc.MAX_ITERATIONS) and rec["reserved"] == len(stages) - 1
        t.set_refine_schedule(psc.parse_schedule(psc.GT_SCHEDULES[0]))
        rec = t.refine_poses(one_match(bx, by, 0), g["scene"], rects=rects, **prc.refine_kwargs(P))[0]
        err = prc.pose_errors(*compose_pose((g["R_a"], g["distance"]), rec), g["R_b"], g["T_b_m"])
        assert rec["rms_last_mm"] < rec["rms_first_mm"] and err[0] < e0[0] and err[1] < e0[1], (err, e0)
    finally:
        t.close()


def test_schedule_cleared_and_the_one_stage_schedule_give_the_unstaged_bytes():
    jobs, scenes = prc.constructed_jobs(), prc.scenes()
    crops = [j.crop for j in jobs]
    rects = np.asarray([(j.rect_xy[0], j.rect_xy[1], j.crop.shape[1], j.crop.shape[0]) for j in jobs], np.int32)
    never, t = DepthTemplates.from_crops(crops), DepthTemplates.from_crops(crops)
    try:
        for k, j in enumerate(jobs):
            kw = prc.refine_kwargs(j.P)
            want = never.refine_poses(one_match(j.x, j.y, k), scenes[j.scene], rects=rects, **kw)
            want_sums = never.debug_pose_refine_sums(scenes[j.scene], one_match(j.x, j.y, k), rects=rects, **kw)[1]
            t.set_refine_schedule(TWO)
            other = t.refine_poses(one_match(j.x, j.y, k), scenes[j.scene], rects=rects, **kw)
            t.set_refine_schedule([psc.stage_of_params(j.P)])
            assert_records(t.refine_poses(one_match(j.x, j.y, k), scenes[j.scene], rects=rects, **kw), want, (j.name, "one stage"))
            assert np.array_equal(t.debug_pose_refine_sums(scenes[j.scene], one_match(j.x, j.y, k), rects=rects, **kw)[1], want_sums), j.name
            t.set_refine_schedule(None)
            assert_records(t.refine_poses(one_match(j.x, j.y, k), scenes[j.scene], rects=rects, **kw), want, (j.name, "cleared"))
            assert np.array_equal(t.debug_pose_refine_sums(scenes[j.scene], one_match(j.x, j.y, k), rects=rects, **kw)[1], want_sums), j.name
            if j.name == "holes":
                assert other.tobytes() != want.tobytes() and other["reserved"][0] == 1                   # the schedule was in force in between
    finally:
        never.close()
        t.close()


def test_seventy_jobs_over_three_frames_and_the_resident_scene(constructed, host):
    t, jobs, scenes, _, rects, index = constructed
    rng = np.random.RandomState(22)
    frames = [scenes[name] for name in ("plain", "holes", "sparse")]
    usable = sorted({index[k] for k, j in enumerate(jobs) if j.crop.shape[0] > 1})
    crop_of = {index[k]: j.crop for k, j in enumerate(jobs)}
    offsets = [0, 30, 30, 70]                                                      # the middle frame has no matches
    m = np.zeros(70, MATCH_DTYPE)
    m["template_id"] = rng.choice(usable, 70)
    m["x"], m["y"] = rects[m["template_id"], 0] + rng.randint(-3, 4, 70), rects[m["template_id"], 1] + rng.randint(-3, 4, 70)
    m["class_index"] = np.arange(70) % 3
    m["template_id"][m["class_index"] == 2] = len(rects) + 7                       # another class's ids are not looked at
    P = prc.make_params(prc.CAM, prc.CAM, max_dist_mm=12.0, max_iterations=5, min_pairs=6, search_radius=1)
    frame_of = np.repeat(np.arange(3), np.diff(offsets))
    t.set_refine_schedule(TWO)
    try:
        for cls in (0, 1):
            got = t.refine_poses(m, frames, offsets, class_index=cls, rects=rects, **prc.refine_kwargs(P))
            second = 0
            for i in range(70):
                if m["class_index"][i] != cls:
                    assert not got[i:i + 1].view(np.uint8).any(), i
                    continue
                k = int(m["template_id"][i])
                want, _ = psc.host_refine_staged(host, P, TWO, crop_of[k], rects[k, :2], frames[frame_of[i]], m["x"][i], m["y"][i], POSE_REFINE_DTYPE)
                assert_records(got[i:i + 1], want, (cls, i))
                second += int(want["reserved"][0] == 1 and want["iterations"][0] > 4)
            assert second >= 8
            t.upload_scene(frames)
            assert_records(t.refine_poses(m, None, offsets, class_index=cls, rects=rects, **prc.refine_kwargs(P)), got, ("resident", cls))
    finally:
        t.set_refine_schedule(None)


def test_pose_chain_under_a_schedule_equals_the_host_composition(host):
    crops, rects = tpc.the_crops()
    t = DepthTemplates.from_crops(crops)
    try:
        scenes = [prc.make_scene(), pvc.paste(crops[0], (30, 20))]
        t.upload_scene(scenes)
        L = pcc.build_lists([(0, tpc.frame_matches(6, rects, 1), [[0, 1], [2], [3, 4, 5]]), (0, tpc.frame_matches(4, rects, 2, templates=(0, 3)), [[0, 2], [1, 3]])])
        plain = tpc.run_hook(t, L, rects)
        t.set_refine_schedule(TWO)
        want = pcc.host_staged(t, L, {0, 1}, 0, tpc.PR, tpc.PV, tpc.THRESH, rects)
        got = tpc.run_hook(t, L, rects)
        p, _ = tpc.check_against_host(got, want, 5, 5, 0, "two stages")
        assert (p["reserved"] == 1).any() and got[2].tobytes() != plain[2].tobytes()
        P = prc.make_params(prc.CAM, prc.CAM, max_dist_mm=12.0, max_iterations=6, min_pairs=3, search_radius=1)
        for k, (lead, pose, _, _) in want.items():                                   # and the composition's refine step is the header's
            mm, f = L.matches[lead], 0 if lead < 6 else 1
            ref, _ = psc.host_refine_staged(host, P, TWO, crops[mm["template_id"]], rects[mm["template_id"], :2], scenes[f], mm["x"], mm["y"], POSE_REFINE_DTYPE)
            assert_records(pose, ref, ("slot", k))
        # a schedule set between two queued calls affects only the second
        stream = torch.cuda.current_stream()
        res = pcc.lists_on_device(L, stream)
        t.set_refine_schedule(None)
        first = t.pose_chain(res, tpc.THRESH, class_index=0, rects=rects, **tpc.KW)
        t.set_refine_schedule(TWO)
        second = t.pose_chain(res, tpc.THRESH, class_index=0, rects=rects, **tpc.KW)
        t.set_refine_schedule(None)
        first, second = first.to_host(), second.to_host()
        assert first[2].tobytes() == plain[2][:5].tobytes() and second[2].tobytes() == got[2][:5].tobytes()
        assert first[3].tobytes() == plain[3][:5].tobytes() and second[3].tobytes() == got[3][:5].tobytes()
    finally:
        t.close()


def test_rough_pose_chain_under_a_schedule_equals_the_host_composition(host):
    tri, views, scene, L = trp.chain_setup()
    model = trp.model_of(views, tri=tri)
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    t2 = None
    stages = psc.parse_schedule("4:8:12:1,1:4:12:1", eps_rot_rad=1e-4, eps_trans_mm=1e-2)
    try:
        t.upload_scene(scene)
        t.set_refine_schedule(stages)
        hdr, rough, group, poses, checks, keep = trp.run_hook(t, model, L, trp.rpc.trace_min_of(10.0), room=2)
        n = len(L.clusters)
        assert hdr[0] == n == 9
        crops = [model.debug_crop(k) for k in range(n)]
        t2 = DepthTemplates.from_crops([c for c, _ in crops])
        t2.upload_scene(scene)
        t2.set_refine_schedule(stages)
        m = pcc.matches_of([(rough["x"][k], rough["y"][k], 90.0, k, 0) for k in range(n)])
        rects = np.asarray([r for _, r in crops], np.int32)
        offsets = [0, 4, 8, 9]
        want_p = t2.refine_poses(m, None, offsets, rects=rects, **trp.PR)
        want_c = t2.verify_poses(m, want_p, None, offsets, rects=rects, **trp.PV)
        assert_records(poses[:n], want_p, "rough chain")
        assert checks[:n].tobytes() == want_c.tobytes() and keep[:n].tolist() == keep_verified(want_c, trp.THRESH).astype(np.uint8).tolist()
        assert (want_p["reserved"] == 1).any() and (want_p["status"] == prc.NO_OVERLAP).any()
        P = prc.make_params(trp.CAM, trp.CAM, max_dist_mm=12.0, eps_rot_rad=1e-4, eps_trans_mm=1e-2, max_iterations=64, min_pairs=3, search_radius=1)
        frame_of = np.repeat(np.arange(3), np.diff(offsets))
        for k in range(n):
            ref, _ = psc.host_refine_staged(host, P, stages, crops[k][0], rects[k, :2], scene[frame_of[k]], m["x"][k], m["y"][k], POSE_REFINE_DTYPE)
            assert_records(poses[k:k + 1], ref, ("slot", k))
    finally:
        model.close()
        t.close()
        if t2 is not None:
            t2.close()


def test_the_setter_next_to_device_work(constructed):
    t, jobs, scenes, want, rects, index = constructed
    k = [j.name for j in jobs].index("crop_33x37_stride_4")
    j = jobs[k]
    t.set_refine_schedule(j.stages)
    for bad in ([dict(j.stages[0], stride=5), j.stages[1]], [dict(j.stages[0], max_iterations=0), j.stages[1]], [dict(j.stages[0], max_dist_mm=float("nan"))], j.stages * 3):
        with pytest.raises(_lib.LmxError) as e:
            t.set_refine_schedule(bad)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG
        assert t.refine_schedule == j.stages
        assert_records(t.refine_poses(one_match(j.x, j.y, index[k]), scenes[j.scene], rects=rects, **prc.refine_kwargs(j.P)), want[k][0], "after a refusal")
    # the per-stage fields of the parameters are still range-checked under a schedule, but not read
    with pytest.raises(_lib.LmxError):
        t.refine_poses(one_match(j.x, j.y, index[k]), scenes[j.scene], rects=rects, **dict(prc.refine_kwargs(j.P), max_iterations=65))
    other = dict(prc.refine_kwargs(j.P), max_iterations=1, max_dist_mm=900.0, search_radius=0, eps_rot_rad=0.5)
    assert_records(t.refine_poses(one_match(j.x, j.y, index[k]), scenes[j.scene], rects=rects, **other), want[k][0], "fields not read")
    # append keeps the destination's schedule
    t.set_refine_schedule(None)
    dst, src = DepthTemplates.from_crops([j.crop]), DepthTemplates.from_crops([jobs[0].crop])
    try:
        dst.set_refine_schedule(j.stages)
        src.set_refine_schedule(TWO)
        dst.append(src)
        assert len(dst) == 2 and dst.refine_schedule == j.stages
        two = np.asarray([rects[index[k]], rects[index[0]]], np.int32)
        assert_records(dst.refine_poses(one_match(j.x, j.y, 0), scenes[j.scene], rects=two, **prc.refine_kwargs(j.P)), want[k][0], "after append")
    finally:
        dst.close()
        src.close()


def test_cpp_caller_prints_what_python_computes(tmp_path):
    """tests/cpp/pose_refine_staged_main.cpp (a crop, a schedule set and read back, the matches refined under it and again without) against
    the same calls here."""
    c, r = prc.make_crop(33, 37, (30, 20))
    scene = prc.make_scene(holes=0.25)
    text = "4:6:12:1,2:3:12:2,1:3:6:0"
    places = [(30, 20), (28, 22), (-9, -11), (prc.SCENE_W, 10)]
    t = DepthTemplates.from_crops([c])
    rects = np.asarray([(r[0], r[1], 33, 37)], np.int32)
    m = np.concatenate([one_match(x, y, 0) for x, y in places])
    kw = dict(model_camera=prc.CAM, scene_camera=prc.CAM, rects=rects)

    def lines(what, poses):
        return ["%s match %d %d status %d stage %d iterations %d pairs %d %d rms %.17g %.17g R %s t %.17g %.17g %.17g"
                % (what, x, y, p["status"], p["reserved"], p["iterations"], p["n_pairs_first"], p["n_pairs_last"], p["rms_first_mm"], p["rms_last_mm"],
                   " ".join("%.17g" % v for v in p["R"].reshape(9)), p["t_mm"][0], p["t_mm"][1], p["t_mm"][2]) for (x, y), p in zip(places, poses)]

    t.set_refine_schedule(psc.parse_schedule(text))
    staged = t.refine_poses(m, scene, **kw)
    t.set_refine_schedule(None)
    single = t.refine_poses(m, scene, **kw)
    t.close()
    assert (staged["reserved"] == 2).any() and staged.tobytes() != single.tobytes()
    want = ["schedule " + " ".join("%d:%d:%.17g:%d" % (st["stride"], st["max_iterations"], st["max_dist_mm"], st["search_radius"]) for st in psc.parse_schedule(text))]
    want += lines("staged", staged) + ["schedule cleared 0"] + lines("single", single)
    exe = str(tmp_path / "pose_refine_staged_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_refine_staged_main.cpp"), "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    np.ascontiguousarray(c).tofile(tmp_path / "crop.u16")
    np.ascontiguousarray(scene).tofile(tmp_path / "scene.u16")
    res = subprocess.run([exe, str(tmp_path / "crop.u16"), "33", "37", str(r[0]), str(r[1]), str(tmp_path / "scene.u16"), str(prc.SCENE_W), str(prc.SCENE_H)]
                         + [repr(v) for v in prc.CAM] + [text] + ["%d,%d" % p for p in places], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want
