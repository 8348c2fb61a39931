"""The scene's depth outlier filter on the device (csrc/lmx_scene_filter.hip: k_scene_filter_score, k_scene_filter_apply; the definition:
csrc/lmx_scene_filter.hpp) through DepthTemplates.set_scene_filter and the hook debug_scene_filtered.  Nothing here has a tolerance:
  the filtered map and the record   equal the CPU build of the header on every frame of tests/scene_filter_cases.py, byte for byte
  the wiring                        with the filter set, refine_poses, verify_poses, debug_pose_chain, debug_rough_pose_chain and pose_chain
                                    return what an object without the setting returns when the read-back filtered frames are its scene
The pose scene is the 12-triangle box of tests/test_gpu_rough_pose.py rendered into frames of 96 x 72 in front of a wall, with pixels on
the box's outline planted midway between the two."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mesh_cases as mc
import pose_chain_cases as pcc
import pose_refine_cases as prc
import pose_verify_cases as pvc
import rough_pose_cases as rpc
import scene_filter_cases as sfc
from conftest import ROOT
from linemod_pose_estimation_amd import DepthTemplates, Detector, NativeBank, _lib, cluster_leaders, keep_verified, meshsynth as ms
from test_gpu_rough_pose import CAM, H, W, chain_setup, model_of

pytestmark = pytest.mark.gpu

THRESH = 0.3
CANARY = 0x5a
PR = prc.refine_kwargs(prc.make_params(CAM, CAM, max_dist_mm=12.0, max_iterations=6, min_pairs=3, search_radius=1))
PV = pvc.verify_kwargs(pvc.make_params(CAM, CAM))
KW = dict(PR, **{k: v for k, v in PV.items() if k not in PR})
WALL_MM = 800


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sfc.build_host(tmp_path_factory.mktemp("sfgpu"))


@pytest.fixture(scope="module")
def plain():
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    yield t
    t.close()


def device_filter(t, frames, cam, r=3, k=15, mul=1.0):
    t.set_scene_filter(r, k, mul, camera=cam)
    t.upload_scene(frames)
    return [t.debug_scene_filtered(f) for f in range(len(frames))]


def check_frames(host, got, frames, cam, r=3, k=15, mul=1.0, what=""):
    for f, (scene, (filtered, info)) in enumerate(zip(frames, got)):
        rc, want, rec = sfc.host_filter(host, scene, cam, r, k, mul)
        assert rc == 0
        assert filtered.tobytes() == want.tobytes(), (what, f, np.argwhere(filtered != want)[:5])
        assert sfc.record_array(info).tobytes() == rec.tobytes(), (what, f, info, rec)


def test_device_equals_the_header_on_the_small_frames(plain, host):
    for name, scene, cam, r, k, mul in sfc.small_cases():
        check_frames(host, device_filter(plain, [scene], cam, r, k, mul), [scene], cam, r, k, mul, name)
    for name, scene, planted in sfc.constructed_scenes():
        cam = sfc.scene_camera(scene)
        got = device_filter(plain, [scene], cam)
        check_frames(host, got, [scene], cam, what=name)
        assert got[0][1]["n_removed"] == len(planted) and got[0][1]["n_sparse"] == 0 and all(got[0][0][p] == 0 for p in planted)
        check_frames(host, device_filter(plain, [scene], cam, k=16), [scene], cam, k=16, what=name + " k 16")


def test_two_frames_keep_their_own_sums_and_a_large_frame(plain, host):
    frames = sfc.two_frames()
    cam = sfc.scene_camera(frames[0])
    got = device_filter(plain, frames, cam)
    check_frames(host, got, frames, cam, what="two frames")
    assert got[0][1]["sum_q"] != got[1][1]["sum_q"] and got[0][1]["threshold"] != got[1][1]["threshold"] and got[0][1]["n_valid"] != got[1][1]["n_valid"]
    for r, k in ((3, 15), (7, 100)):       # 321 x 241: 11 x 31 = 341 tiles, the last column and row of them cut, one tile per workgroup (later trips: test_gpu_second_trips.py)
        big = sfc.large_frame()
        cam = sfc.scene_camera(big)
        got = device_filter(plain, [big], cam, r, k)
        check_frames(host, got, [big], cam, r, k, what="321 x 241 r %d" % r)
        assert got[0][1]["n_removed"] > 0 and got[0][1]["n_scored"] > 0


def test_new_upload_and_new_setting_recompute_and_none_restores(plain, host):
    a, b = sfc.noisy(45, 35, 11), sfc.noisy(45, 35, 12)
    cam = sfc.scene_camera(a)
    first = device_filter(plain, [a], cam)
    check_frames(host, first, [a], cam, what="first scene")
    plain.upload_scene([b])                                              # a new scene under the same setting
    second = [plain.debug_scene_filtered(0)]
    check_frames(host, second, [b], cam, what="second scene")
    assert first[0][0].tobytes() != second[0][0].tobytes()
    plain.set_scene_filter(2, 9, 0.5, camera=cam)                        # a new setting on the same scene
    check_frames(host, [plain.debug_scene_filtered(0)], [b], cam, 2, 9, 0.5, what="new setting")
    plain.set_scene_filter(None)
    with pytest.raises(_lib.LmxError):
        plain.debug_scene_filtered(0)


# ---- the wiring -----------------------------------------------------------------------------------------------------------------------------------

def plant(frame, every=3):
    """The rendered frame in front of a wall, every `every`-th background pixel that touches the object planted midway -> (frame, n planted)."""
    obj = frame != 0
    out = np.where(obj, frame, WALL_MM).astype(np.uint16)
    near = np.zeros_like(obj)
    near[1:, :] |= obj[:-1, :]
    near[:-1, :] |= obj[1:, :]
    near[:, 1:] |= obj[:, :-1]
    near[:, :-1] |= obj[:, 1:]
    outline = np.argwhere(near & ~obj)[::every]
    for y, x in outline:
        out[y, x] = (int(frame[obj].mean()) + WALL_MM) // 2
    return out, len(outline)


@pytest.fixture(scope="module")
def setup():
    """The filtered object `a` (raw frames resident), the plain object `b` (the read-back filtered frames resident), the frames, lists, model"""
    tri, views, scene, L = chain_setup()
    planted = [plant(s) for s in scene[:2]]
    raw = [p[0] for p in planted] + [np.full((H, W), WALL_MM, np.uint16)]
    a = DepthTemplates.from_mesh(tri, views.pairs(), W, H, *CAM)
    b = DepthTemplates.from_mesh(tri, views.pairs(), W, H, *CAM)
    model = model_of(views, tri=tri)
    a.set_scene_filter(camera=CAM)
    a.upload_scene(raw)
    filtered, infos = zip(*[a.debug_scene_filtered(f) for f in range(3)])
    for f in range(2):                                                   # the filter took part: planted pixels went, the object stayed
        assert infos[f]["n_removed"] > 0 and (filtered[f] != raw[f]).any() and planted[f][1] > 0, (f, infos[f], planted[f][1])
    b.upload_scene(list(filtered))
    yield a, b, raw, [np.ascontiguousarray(f) for f in filtered], L, model
    a.close()
    b.close()
    model.close()


def offsets_of(L):
    return [int(v) for v in L.frame_info[:, 0]] + [len(L.matches)]


def same(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_refine_and_verify_equal_the_plain_object_on_filtered_frames(setup):
    a, b, raw, filtered, L, _ = setup
    m, offs = L.matches, offsets_of(L)
    pa, pb = a.refine_poses(m, None, offs, **PR), b.refine_poses(m, None, offs, **PR)                      # resident
    assert same(pa, pb) and (pa["status"] != prc.NONE).any()
    ca, cb = a.verify_poses(m, pa, None, offs, **PV), b.verify_poses(m, pb, None, offs, **PV)
    assert same(ca, cb) and (ca["status"] == pvc.OK).any()
    plain = DepthTemplates.from_crops([a.crop(i) for i in range(len(a))])                                   # the same crops, no setting, the raw frames
    try:
        rects = np.asarray([a.rect(i) for i in range(len(a))], np.int32)
        praw = plain.refine_poses(m, raw, offs, rects=rects, **PR)
        craw = plain.verify_poses(m, praw, raw, offs, rects=rects, **PV)
        assert not same(praw, pa) and not same(craw, ca)                                                    # the filter demonstrably took part
        # staged frames: the filtered object given the raw frames, the plain one given the filtered frames
        sa, sb = a.refine_poses(m, raw, offs, **PR), plain.refine_poses(m, filtered, offs, rects=rects, **PR)
        assert same(sa, sb) and same(sa, pa)
        va, vb = a.verify_poses(m, sa, raw, offs, **PV), plain.verify_poses(m, sb, filtered, offs, rects=rects, **PV)
        assert same(va, vb) and same(va, ca)
    finally:
        plain.close()
    a.upload_scene(raw)                                                  # the staged calls forgot the scenes: put them back for the tests below
    b.upload_scene(filtered)
    # off again: the raw bytes
    a.set_scene_filter(None)
    assert same(a.refine_poses(m, None, offs, **PR), praw)
    a.set_scene_filter(camera=CAM)
    assert same(a.refine_poses(m, None, offs, **PR), pa)


def test_chain_hooks_equal_the_plain_object_on_filtered_frames(setup):
    a, b, raw, filtered, L, model = setup
    out = []
    for t in (a, b):
        chain = t.debug_pose_chain(L.header, L.frame_info, L.matches, L.clusters, L.members, THRESH, fill=CANARY, class_index=0, **KW)
        rough = t.debug_rough_pose_chain(model, L.header, L.frame_info, L.matches, L.clusters, L.members, THRESH, trace_min=rpc.trace_min_of(10.0), fill=CANARY, **KW)
        out.append((chain, rough))
    for ga, gb in zip(out[0], out[1]):
        assert len(ga) == len(gb) and all(same(x, y) for x, y in zip(ga, gb))
    hdr, leaders, poses, checks, keep = out[0][0]
    assert hdr[0] == len(L.clusters) and hdr[2] > 0 and hdr[3] > 0
    a.set_scene_filter(None)                                             # against the raw scene the records differ
    try:
        raw_chain = a.debug_pose_chain(L.header, L.frame_info, L.matches, L.clusters, L.members, THRESH, fill=CANARY, class_index=0, **KW)
        raw_rough = a.debug_rough_pose_chain(model, L.header, L.frame_info, L.matches, L.clusters, L.members, THRESH, trace_min=rpc.trace_min_of(10.0), fill=CANARY, **KW)
    finally:
        a.set_scene_filter(camera=CAM)
    assert not same(raw_chain[2], poses) and not same(raw_chain[3], checks)
    assert not same(raw_rough[3], out[0][1][3]) and same(raw_rough[1], out[0][1][1])                        # the rough stage reads no scene


def test_pose_chain_on_an_export_equals_the_plain_object_on_filtered_frames(setup):
    a, b, raw, filtered, L, _ = setup
    stream = torch.cuda.current_stream()
    res = pcc.lists_on_device(L, stream)
    ga = a.pose_chain(res, THRESH, class_index=0, **KW).to_host()
    gb = b.pose_chain(res, THRESH, class_index=0, **KW).to_host()
    assert all(same(x, y) for x, y in zip(ga, gb)) and ga[0][0] == len(L.clusters) and ga[0][2] > 0
    hook = a.debug_pose_chain(L.header, L.frame_info, L.matches, L.clusters, L.members, THRESH, fill=CANARY, class_index=0, **KW)
    n = int(ga[0][0])
    assert same(ga[2][:n], hook[2][:n]) and same(ga[3][:n], hook[3][:n])                                    # the hook's poses and checks, slot for slot
    times = None
    a.set_profiling(True)
    try:
        a.upload_scene(raw)                                              # a new scene: the next chain call makes the copy again, once
        a.pose_chain(res, THRESH, class_index=0, **KW).to_host()
        a.pose_chain(res, THRESH, class_index=0, **KW).to_host()
        times = a.kernel_times()
    finally:
        a.set_profiling(False)
    assert times["k_scene_filter_score"][1] == 1 and times["k_scene_filter_apply"][1] == 1 and times["k_pose_refine_clusters"][1] == 2
    b.set_profiling(True)
    try:
        b.pose_chain(res, THRESH, class_index=0, **KW).to_host()
        times = b.kernel_times()
    finally:
        b.set_profiling(False)
    assert times["k_scene_filter_score"][1] == 0 and times["k_scene_filter_apply"][1] == 0                 # never set: nothing of it is launched


def test_cpp_caller_prints_what_python_computes(tmp_path):
    """tests/cpp/scene_filter_chain_main.cpp -- train from a mesh, setSceneFilter, upload the frame to the device, enqueue, upload the scene,
    export the depth-scored clusters, DepthTemplates::poseChain, one synchronisation to print -- against the host-staged path from Python
    with the same setting on the same scene: the workload of tests/test_gpu_pose_chain_cpp.py with every fourth pixel of the depth edges
    pulled 60 mm towards the camera."""
    exe = str(tmp_path / "scene_filter_chain_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scene_filter_chain_main.cpp"), "-o", exe, "-L", _lib.CSRC, "-llmx", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    Wc, Hc, F, threshold = 320, 240, ms.ENSENSO["fx"] / 2, 75.0
    cam = (F, F, Wc / 2.0, Hc / 2.0)
    chip, cpu = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary")
    views = ms.view_grid()[:204]
    b = ms.empty_bank()
    nb = NativeBank.create(b.T, b.modalities)
    nb.train_mesh(chip, views, Wc, Hc, F, F)
    sc = nb.last_side_car
    sources, _ = ms.make_scene(chip, views, width=Wc, height=Hc, seed=11, n_instances=2, fx=F, fy=F, other_tri=cpu, n_other=1, margin=44)
    color, depth = np.ascontiguousarray(sources[0]), np.ascontiguousarray(sources[1]).copy()
    left, right = depth[:, :-1].astype(np.int64), depth[:, 1:].astype(np.int64)
    edges = np.argwhere((np.abs(left - right) > 8) & (left > 0) & (right > 0))[::4]
    assert len(edges) > 50
    for y, x in edges:
        depth[y, x] -= 60
    t = DepthTemplates.from_mesh(chip, list(zip(sc["R"], sc["T"][:, 2])), Wc, Hc, F, F)
    det = Detector(nb, Wc, Hc, max_candidates=1 << 17)
    try:
        t.set_scene_filter(camera=cam)
        det.set_cluster_sidecar(sc["obj_origin_dists"], sc["rects"], 10, 0.4, 0.05, 2)
        det.upload([[color, depth]])
        det.enqueue(1, threshold)
        t.upload_scene([depth])
        matches, _, clusters, members = det.collect_clusters_depth(1, t, cap_total=1 << 17)[0]
        lead = cluster_leaders(clusters, members, matches)
        assert len(lead) >= 1
        poses = t.refine_poses(matches[lead], None, model_camera=cam, scene_camera=cam)
        checks = t.verify_poses(matches[lead], poses, None, model_camera=cam, scene_camera=cam)
        keep = keep_verified(checks, THRESH)
        filtered, info = t.debug_scene_filtered(0)
        t.set_scene_filter(None)
        raw_poses = t.refine_poses(matches[lead], None, model_camera=cam, scene_camera=cam)
    finally:
        det.close()
        t.close()
    assert info["n_removed"] >= len(edges) and all(filtered[y, x] == 0 for y, x in edges) and poses.tobytes() != raw_poses.tobytes()
    want = ["filter valid %d sparse %d scored %d removed %d sum_q %d sum_qq %d threshold %.17g zeroed %d"
            % (info["n_valid"], info["n_sparse"], info["n_scored"], info["n_removed"], info["sum_q"], info["sum_qq"], info["threshold"], int(((depth != 0) & (filtered == 0)).sum())),
            "templates %d matches %d clusters %d status 0" % (len(sc["rects"]), len(matches), len(clusters)),
            "chain live %d flags 0 refined %d verified %d kept %d" % (len(clusters), int((poses["status"] != 0).sum()), int((checks["status"] == pvc.OK).sum()), int(keep.sum()))]
    for k, (i, p, v) in enumerate(zip(lead, poses, checks)):
        m = matches[i]
        want.append("cluster %d leader %d %d %d pose status %d iterations %d t %.17g %.17g %.17g verify status %d points %d %d %d scene %d cells %d roi %d %d %d %d rate %.17g %s"
                    % (k, m["x"], m["y"], m["template_id"], p["status"], p["iterations"], p["t_mm"][0], p["t_mm"][1], p["t_mm"][2], v["status"], v["n_model"], v["n_tested"],
                       v["n_occupied"], v["n_scene"], v["cells"], v["roi"][0], v["roi"][1], v["roi"][2], v["roi"][3], v["rate"], "kept" if keep[k] else "erased"))
    np.ascontiguousarray(chip, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(views).tofile(tmp_path / "views.f64")
    color.tofile(tmp_path / "bgr.u8")
    depth.tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), str(Wc), str(Hc), repr(F), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"),
                          repr(threshold), repr(THRESH)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want
