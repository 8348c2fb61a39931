"""The pose chain end to end from C++: tests/cpp/pose_chain_main.cpp (train from a mesh, upload the frame to the device, enqueue, upload the
scene, export the depth-scored clusters, DepthTemplates::poseChain, print what is kept -- one synchronisation, only to print) against the
host-staged path from Python on the same scene: collect_clusters_depth -> cluster_leaders -> refine_poses -> verify_poses -> keep_verified."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import pose_verify_cases as pvc
from conftest import ROOT
from linemod_pose_estimation_amd import DepthTemplates, Detector, NativeBank, _lib, cluster_leaders, keep_verified, meshsynth as ms

pytestmark = pytest.mark.gpu

F = ms.ENSENSO["fx"]
W, H = 320, 240
THRESHOLD = 75.0
COLLISION_RATE_THRESHOLD = 0.3       # the carmine node's default


def test_cpp_caller_prints_what_python_computes(tmp_path):
    exe = str(tmp_path / "pose_chain_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_chain_main.cpp"), "-o", exe, "-L", _lib.CSRC, "-llmx", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    chip, cpu = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary")
    views = ms.view_grid()[:204]
    b = ms.empty_bank()
    nb = NativeBank.create(b.T, b.modalities)
    nb.train_mesh(chip, views, W, H, F / 2, F / 2)
    sc = nb.last_side_car
    sources, _ = ms.make_scene(chip, views, width=W, height=H, seed=11, n_instances=2, fx=F / 2, fy=F / 2, other_tri=cpu, n_other=1, margin=44)
    template_views = list(zip(sc["R"], sc["T"][:, 2]))
    t = DepthTemplates.from_mesh(chip, template_views, W, H, F / 2, F / 2)
    det = Detector(nb, W, H, max_candidates=1 << 17)
    det.set_cluster_sidecar(sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
    det.upload([[np.ascontiguousarray(s) for s in sources]])
    det.enqueue(1, THRESHOLD)
    t.upload_scene([sources[1]])
    matches, _, clusters, members = det.collect_clusters_depth(1, t, cap_total=1 << 17)[0]
    det.close()
    lead = cluster_leaders(clusters, members, matches)
    assert len(lead) >= 1
    cam = (F / 2, F / 2, W / 2.0, H / 2.0)
    poses = t.refine_poses(matches[lead], None, model_camera=cam, scene_camera=cam)
    checks = t.verify_poses(matches[lead], poses, None, model_camera=cam, scene_camera=cam)
    keep = keep_verified(checks, COLLISION_RATE_THRESHOLD)
    t.close()
    assert (checks["status"] == pvc.OK).all() and keep.any()
    want = ["templates %d matches %d clusters %d status 0" % (len(sc["rects"]), len(matches), len(clusters)),
            "chain live %d flags 0 refined %d verified %d kept %d" % (len(clusters), int((poses["status"] != 0).sum()), int((checks["status"] == pvc.OK).sum()), int(keep.sum()))]
    for k, (i, p, v) in enumerate(zip(lead, poses, checks)):
        m = matches[i]
        want.append("cluster %d leader %d %d %d pose status %d iterations %d t %.17g %.17g %.17g verify status %d points %d %d %d scene %d cells %d roi %d %d %d %d rate %.17g %s"
                    % (k, m["x"], m["y"], m["template_id"], p["status"], p["iterations"], p["t_mm"][0], p["t_mm"][1], p["t_mm"][2], v["status"], v["n_model"], v["n_tested"],
                       v["n_occupied"], v["n_scene"], v["cells"], v["roi"][0], v["roi"][1], v["roi"][2], v["roi"][3], v["rate"], "kept" if keep[k] else "erased"))
    np.ascontiguousarray(chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(views).tofile(tmp_path / "views.f64")
    np.ascontiguousarray(sources[0]).tofile(tmp_path / "bgr.u8")
    np.ascontiguousarray(sources[1]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(W), str(H), repr(F / 2), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(THRESHOLD), repr(COLLISION_RATE_THRESHOLD)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want
