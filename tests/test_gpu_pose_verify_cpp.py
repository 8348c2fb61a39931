"""Pose verification end to end: tests/cpp/pose_verify_main.cpp (train from a mesh, match, cluster, refine each cluster's leader, verify,
print what is kept) against the same chain from Python, and the decision the stage exists for -- the true match of a rendered golden
mesh is kept at the reference's threshold, the same match against a scene without the object is erased."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import pose_refine_cases as prc
import pose_verify_cases as pvc
from conftest import ROOT
from linemod_pose_estimation_amd import (MATCH_DTYPE, DepthTemplates, Detector, NativeBank, _lib, cluster_leaders, cluster_matches_scored, depth_values, keep_verified,
                                         meshsynth as ms)

pytestmark = pytest.mark.gpu

F = ms.ENSENSO["fx"]
W, H = 320, 240
THRESHOLD = 75.0
COLLISION_RATE_THRESHOLD = 0.3       # the carmine node's default


def test_cpp_caller_prints_what_python_computes(tmp_path):
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
    t.upload_scene([sources[1]])
    poses = t.refine_poses(matches[lead], None, model_camera=cam, scene_camera=cam)
    checks = t.verify_poses(matches[lead], poses, None, model_camera=cam, scene_camera=cam)
    keep = keep_verified(checks, COLLISION_RATE_THRESHOLD)
    assert (checks["status"] == pvc.OK).all() and (checks["n_scene"] > 0).any() and keep.any()
    want = ["templates %d matches %d clusters %d" % (len(sc["rects"]), len(matches), len(clusters))]
    for k, (i, p, v) in enumerate(zip(lead, poses, checks)):
        m = matches[i]
        want.append("cluster %d leader %d %d %d pose status %d verify status %d points %d %d %d scene %d cells %d roi %d %d %d %d rate %.17g %s"
                    % (k, m["x"], m["y"], m["template_id"], p["status"], v["status"], v["n_model"], v["n_tested"], v["n_occupied"], v["n_scene"], v["cells"],
                       v["roi"][0], v["roi"][1], v["roi"][2], v["roi"][3], v["rate"], "kept" if keep[k] else "erased"))
    t.close()
    exe = str(tmp_path / "pose_verify_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_verify_main.cpp"),
                           "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    np.ascontiguousarray(chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(views).tofile(tmp_path / "views.f64")
    np.ascontiguousarray(sources[0]).tofile(tmp_path / "bgr.u8")
    np.ascontiguousarray(sources[1]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(W), str(H), repr(F / 2), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(THRESHOLD), repr(COLLISION_RATE_THRESHOLD)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want


def test_true_match_is_kept_and_dropped_without_the_object():
    g = prc.ground_truth_case()
    t = DepthTemplates.from_crops([g["crop"]])
    rects = np.asarray([g["rect"]], np.int32)
    m = np.zeros(1, MATCH_DTYPE)
    m["x"], m["y"], m["similarity"] = g["rect"][0], g["rect"][1], 95.0
    cams = dict(model_camera=prc.GT_CAM, scene_camera=prc.GT_CAM)
    n_model = int((g["crop"] != 0).sum())
    # the scene is the render the template was cut from: the true pose
    pose = t.refine_poses(m, g["scene_a"], rects=rects, **cams)
    assert pose["status"][0] == prc.CONVERGED
    there = t.verify_poses(m, pose, g["scene_a"], rects=rects, **cams)
    assert there["status"][0] == pvc.OK and there["n_model"][0] == n_model and there["rate"][0] > 0.9
    assert keep_verified(there, COLLISION_RATE_THRESHOLD).tolist() == [True]
    # the same render at the second pose (2.5 degrees, a few mm): the refined pose keeps it as well
    bx, by = g["rect_b"][:2]
    m2 = m.copy()
    m2["x"], m2["y"] = bx, by
    pose_b = t.refine_poses(m2, g["scene"], rects=rects, **cams)
    moved = t.verify_poses(m2, pose_b, g["scene"], rects=rects, **cams)
    assert keep_verified(moved, COLLISION_RATE_THRESHOLD).tolist() == [True]
    # the same match and pose where the object is not: the table it stood on, 60 mm behind its farthest point
    without = np.full_like(g["scene_a"], int(g["crop"].max()) + 60)
    gone = t.verify_poses(m, pose, without, rects=rects, **cams)
    assert gone["status"][0] == pvc.OK and gone["n_tested"][0] == n_model and gone["n_occupied"][0] == 0
    assert keep_verified(gone, COLLISION_RATE_THRESHOLD).tolist() == [False]
    nothing = t.verify_poses(m, pose, np.zeros_like(g["scene_a"]), rects=rects, **cams)
    assert nothing["n_scene"][0] == 0 and keep_verified(nothing, COLLISION_RATE_THRESHOLD).tolist() == [False]
    t.close()
