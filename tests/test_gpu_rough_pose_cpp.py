"""The rough pose chain end to end from C++: tests/cpp/rough_pose_chain_main.cpp (train from a mesh, upload the frame to the device,
enqueue, upload the scene, export the depth-scored clusters, DepthTemplates::roughPoseChain, print -- one synchronisation, only to print)
against the hook from Python on the same scene's collected lists: collect_clusters_depth -> debug_rough_pose_chain."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import pose_chain_cases as pcc
from conftest import ROOT
from linemod_pose_estimation_amd import DepthTemplates, Detector, NativeBank, RoughModel, _lib, meshsynth as ms

pytestmark = pytest.mark.gpu

F = ms.ENSENSO["fx"]
W, H = 320, 240
THRESHOLD = 75.0
COLLISION_RATE_THRESHOLD = 0.3       # the carmine node's default
ORIENTATION_THRESHOLD_DEG = 10.0
WINDOW = 160


def test_cpp_caller_prints_what_python_computes(tmp_path):
    exe = str(tmp_path / "rough_pose_chain_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rough_pose_chain_main.cpp"), "-o", exe, "-L", _lib.CSRC, "-llmx", "-L", "/opt/rocm/lib", "-lamdhip64",
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
    model = RoughModel(chip, template_views, W, H, F / 2, F / 2, ori_dists=sc["obj_origin_dists"], cap_slots=256, max_window=(WINDOW, WINDOW))
    det = Detector(nb, W, H, max_candidates=1 << 17)
    det.set_cluster_sidecar(sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
    det.upload([[np.ascontiguousarray(s) for s in sources]])
    det.enqueue(1, THRESHOLD)
    t.upload_scene([sources[1]])
    matches, _, clusters, members = det.collect_clusters_depth(1, t, cap_total=1 << 17)[0]
    det.close()
    assert len(clusters) >= 1
    L = pcc.build_lists([(0, matches, [members[c["member_begin"]:c["member_begin"] + c["member_count"]] for c in clusters])])
    cam = (F / 2, F / 2, W / 2.0, H / 2.0)
    hdr, rough, _, poses, checks, keep = t.debug_rough_pose_chain(model, L.header, L.frame_info, L.matches, L.clusters, L.members, COLLISION_RATE_THRESHOLD,
                                                                  threshold_deg=ORIENTATION_THRESHOLD_DEG, scene_camera=cam)
    model.close()
    t.close()
    assert (rough["status"] == 1).any() and hdr[0] == len(clusters)
    want = ["templates %d matches %d clusters %d status 0" % (len(sc["rects"]), len(matches), len(clusters)),
            "chain live %d flags %d refined %d verified %d kept %d rough %d" % tuple(int(v) for v in hdr[:6])]
    for k, (r, p, v) in enumerate(zip(rough, poses, checks)):
        want.append("cluster %d rough status %d members %d groups %d group %d of %d front %d at %d %d distance %.17g R0 %.17g rect %d %d %d %d points %d "
                    "pose status %d iterations %d t %.17g %.17g %.17g verify status %d points %d %d %d rate %.17g %s"
                    % (k, r["status"], r["n_members"], r["n_groups"], r["group"], r["n_group_members"], r["front"], r["x"], r["y"], r["distance"], r["R"][0], r["rect"][0],
                       r["rect"][1], r["rect"][2], r["rect"][3], r["n_model"], p["status"], p["iterations"], p["t_mm"][0], p["t_mm"][1], p["t_mm"][2], v["status"],
                       v["n_model"], v["n_tested"], v["n_occupied"], v["rate"], "kept" if keep[k] else "erased"))
    np.ascontiguousarray(chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(views).tofile(tmp_path / "views.f64")
    np.ascontiguousarray(sources[0]).tofile(tmp_path / "bgr.u8")
    np.ascontiguousarray(sources[1]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(W), str(H), repr(F / 2), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(THRESHOLD), repr(COLLISION_RATE_THRESHOLD), repr(ORIENTATION_THRESHOLD_DEG), str(WINDOW)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want
