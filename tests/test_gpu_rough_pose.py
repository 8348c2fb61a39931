"""lmx_rough_pose_chain_on (csrc/lmx_rough.hip: k_rough_group, k_rough_setup, k_rough_raster, k_rough_finish; csrc/lmx_verify.hip:
k_rough_refine_clusters, k_rough_verify_clusters; the definition: csrc/lmx_rough_pose.hpp) through DepthTemplates.rough_pose_chain, the hook
DepthTemplates.debug_rough_pose_chain and RoughModel.debug_crop.  Nothing here has a tolerance:
  the records and member groups    equal the CPU build of the header on every case of tests/rough_pose_cases.py, byte for byte
  the render                       equals lmx_mesh_render (itself pinned to meshraster.c) at the record's view
  the poses, checks, keep          equal the existing refine_poses -> verify_poses -> keep_verified on the read-back crops and rects
Frames of 96 x 72, a 12-triangle box and a tetrahedron, 16 slots, a window of 64 x 64; and the constructed meshes of tests/mesh_cases.py
that fill more than one staging chunk, on their own 75 x 41 camera."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_cases as mc
import pose_chain_cases as pcc
import pose_refine_cases as prc
import pose_verify_cases as pvc
import rough_pose_cases as rpc
from linemod_pose_estimation_amd import POSE_REFINE_DTYPE, DepthTemplates, ExportedRoughPoses, RoughModel, _lib, keep_verified, render_views
from linemod_pose_estimation_amd.detector import _chain_inputs, _chain_outputs
from rough_pose_cases import EMPTY, FLAG_ROUGH, INVALID_VIEW, JOB, OK, WINDOW_TOO_LARGE, rot
from test_gpu_export_clusters import FX, FY, N_T, S, cfg, export, scene_of, upload_enqueue  # noqa: F401  (cfg is a fixture)

pytestmark = pytest.mark.gpu

W, H, F = 96, 72, 300.0
CAM = (F, F, W / 2.0, H / 2.0)
CANARY = 0x5a
THRESH = 0.3
SLOTS, WINDOW = 16, (64, 64)
PR = prc.refine_kwargs(prc.make_params(CAM, CAM, max_dist_mm=12.0, eps_rot_rad=1e-4, eps_trans_mm=1e-2, max_iterations=64, min_pairs=3, search_radius=1))
PV = pvc.verify_kwargs(pvc.make_params(CAM, CAM))
KW = dict(PR, **{k: v for k, v in PV.items() if k not in PR})
CASES = rpc.cases()


def model_of(views, tri=None, cam=CAM, **kw):
    kw.setdefault("cap_slots", SLOTS)
    kw.setdefault("max_window", WINDOW)
    return RoughModel(rpc.box_mesh() if tri is None else tri, views.pairs(), W, H, cam[0], cam[1], cam[2], cam[3], D=views.D, ori_dists=views.ori_dist, **kw)


def run_hook(t, model, L, trace_min, caps=None, room=2, **kw):
    """debug_rough_pose_chain on L cut to caps, with room for `room` clusters more than the lists hold"""
    caps = caps or (len(L.matches), len(L.clusters), len(L.members))
    clusters = np.concatenate([L.clusters[:caps[1]], L.clusters[:room]])
    args = dict(KW, trace_min=float(trace_min), cap_clusters=caps[1] + room if caps[1] == len(L.clusters) else caps[1], fill=CANARY)
    args.update(kw)
    return t.debug_rough_pose_chain(model, L.header, L.frame_info, L.matches[:caps[0]], clusters, L.members[:caps[2]], THRESH, **args)


@pytest.fixture(scope="module")
def blank():
    """An object whose resident scene is two empty frames: the stage in front of the pose kernels does not look at it"""
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    t.upload_scene([np.zeros((H, W), np.uint16)] * 2)
    yield t
    t.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("rpgpu")
    return rpc.build_host(d), d


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_records_and_groups_equal_the_cpu_build(blank, host, case):
    n_live, hflags, states, flags, recs, group, _ = rpc.run_host(*host, case.L, case.views, case.trace_min, class_index=case.class_index, caps=case.caps)
    case.expect(states, flags, recs, group, case.L)
    model = model_of(case.views)
    try:
        hdr, rough, got_group, poses, checks, keep = run_hook(blank, model, case.L, case.trace_min, caps=case.caps, class_index=case.class_index)
    finally:
        model.close()
    assert got_group.tobytes() == group.tobytes()
    n_ok = 0
    for k in range(len(rough)):
        one = rough[k:k + 1]
        if k >= n_live:                                                  # not written: every byte still the canary
            assert all((a[k:k + 1].view(np.uint8) == CANARY).all() for a in (rough, poses, checks, keep)), k
            continue
        assert one.tobytes()[:128] == recs[k:k + 1].tobytes()[:128], (k, one, recs[k])
        if recs["status"][k] != OK:
            assert one.tobytes() == recs[k:k + 1].tobytes(), (k, one, recs[k])
        else:
            assert one["status"][0] in (OK, INVALID_VIEW, WINDOW_TOO_LARGE, EMPTY), one
            assert (one["n_model"][0] > 0 and one["rect"][0, 2] > 0) if one["status"][0] == OK else not (one["rect"].any() or one["n_model"].any())
        n_ok += int(one["status"][0] == OK)
        if one["status"][0] != OK:                                       # the scene is empty: an OK slot is refined to "no overlap", nothing else is touched
            assert not poses[k:k + 1].view(np.uint8).any() and not checks[k:k + 1].view(np.uint8).any() and keep[k] == 0, k
    want_flags = hflags
    for s, f in zip(states, flags):
        want_flags |= f
    rough_flag = FLAG_ROUGH if any(s == JOB and rough["status"][k] != OK for k, s in enumerate(states)) else 0
    assert hdr[0] == n_live and hdr[1] == (want_flags | rough_flag) and hdr[5] == n_ok and not hdr[6:].any(), (hdr, want_flags)


# ---- the render ----------------------------------------------------------------------------------------------------------------------------------
def render_table():
    """16 views: 12 of the object as a whole at 0.45 .. 0.6 m, then one too near for the window, one that reaches behind Z = 0.01, two spares"""
    R = [rot("y", 25.0 * (k % 4)) @ rot("x", 20.0 + 15.0 * (k // 4)) @ rot("z", 7.0 * k) for k in range(12)]
    R += [rot("x", 30.0), rot("y", 10.0), rot("x", 31.0), rot("y", 11.0)]
    dist = [0.45 + 0.0125 * k for k in range(12)] + [0.2, 0.02, 0.2, 0.02]
    return rpc.Views(R, dist)


def render_lists():
    """14 clusters: each of the 12 whole views alone; the near view with its spare (a mean of three); the view behind the camera with its
    spare"""
    ids = [[k] for k in range(12)] + [[12, 14, 12]] + [[13, 15]]
    return rpc.members_lists(ids, extra_front=False, tail_frame=True)


@pytest.mark.parametrize("mesh,cam", [("box", CAM), ("tetrahedron", CAM), ("box", (F, F, 6.0, H / 2.0)), ("box", (F, F, W / 2.0, H - 5.0))],
                         ids=["box", "tetrahedron", "box_left_border", "box_bottom_border"])
def test_render_equals_lmx_mesh_render(blank, mesh, cam):
    tri = rpc.box_mesh() if mesh == "box" else rpc.tetrahedron(0.05)
    views, L = render_table(), render_lists()
    model = model_of(views, tri=tri, cam=cam)
    try:
        assert model.device_bytes() >= SLOTS * (64 * 64 * 2 + len(tri) * 96)
        hdr, rough, group, _, _, _ = run_hook(blank, model, L, rpc.trace_min_of(5.0), room=0, model_camera=cam, scene_camera=cam)
        crops = [model.debug_crop(k) for k in range(14)]
    finally:
        model.close()
    assert rough["status"][:12].tolist() == [OK] * 12 and rough["status"][12] == WINDOW_TOO_LARGE and rough["status"][13] == INVALID_VIEW
    assert hdr[0] == 14 and hdr[1] == FLAG_ROUGH and hdr[5] == 12
    assert rough["n_group_members"][12] == 3 and rough["n_group_members"][13] == 2
    touches = False
    for k in range(14):
        crop, rect = crops[k]
        if rough["status"][k] != OK:
            assert crop.size == 0 and not rect.any() and not rough["rect"][k].any() and rough["n_model"][k] == 0
            continue
        _, depth, _, rects = render_views(tri, [(rough["R"][k].reshape(3, 3), float(rough["distance"][k]))], W, H, cam[0], cam[1], cam[2], cam[3])
        x, y, w, h = (int(v) for v in rects[0])
        assert rect.tolist() == [x, y, w, h] == rough["rect"][k].tolist(), (k, rect, rects[0])
        assert crop.tobytes() == np.ascontiguousarray(depth[0, y:y + h, x:x + w]).tobytes(), k
        outside = depth[0].copy()
        outside[y:y + h, x:x + w] = 0
        assert not outside.any() and rough["n_model"][k] == np.count_nonzero(depth[0]) > 0, k
        touches = touches or x == 0 or y + h == H
    assert touches == (cam != CAM)


@pytest.mark.parametrize("name", ["roof_ab_after_255", "roof_ab_after_256", "roof_fan_600_order_0"])
def test_render_of_constructed_meshes_equals_lmx_mesh_render(blank, name):
    """More than one staging chunk of 256 records in k_rough_raster (the box and the tetrahedron never fill one): the roof whose two faces
    sit at the indices 255, 256 (the last slot of chunk 0 and the first of chunk 1) and 256, 257, and 600 faces on one ridge (three
    chunks, hits in every wave).  One view, the identity at distance 1; one cluster of one match, so the slot's view is that view bit for
    bit (the mean of one unit quaternion: the CPU build of the header, rough_pose_cases.run_host, gives the same), and the window is the whole 75 x 41
    frame.  The render equals lmx_mesh_render's at the record's view and meshraster.c's (mesh_cases.constructed_expected) on every pixel,
    the ridge's 33 exact z ties included.  What this can show is a record that is never walked or staged in a wrong slot (a walk that stops
    after its first chunk fails all three cases).  Which face wins a tie it cannot show: this path stores depth alone, and equal z is equal
    depth (a walk that lets the higher index win, or stages the waves in reverse order, passes; tests/test_gpu_mesh_render_constructed.py
    sees both through the gray of the same shared walk)."""
    _, tri, cam, _ = next(c for c in mc.constructed_cases() if c[0] == name)
    Wc, Hc, camt = cam["width"], cam["height"], (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    views = rpc.Views([np.eye(3)], 1.0)
    L = rpc.members_lists([[0]], extra_front=False, tail_frame=True)
    model = RoughModel(tri, views.pairs(), Wc, Hc, *camt, D=views.D, ori_dists=views.ori_dist, cap_slots=4, max_window=(Wc, Hc))
    try:
        hdr, rough, _, _, _, _ = run_hook(blank, model, L, rpc.trace_min_of(5.0), room=0, model_camera=camt, scene_camera=camt)
        crop, rect = model.debug_crop(0)
    finally:
        model.close()
    assert hdr[0] == 1 and hdr[1] == 0 and hdr[5] == 1 and rough["status"][0] == OK
    assert rough["R"][0].tobytes() == np.eye(3).tobytes() and rough["distance"][0] == 1.0
    _, depth, _, rects = render_views(tri, [(rough["R"][0].reshape(3, 3), float(rough["distance"][0]))], Wc, Hc, *camt)
    x, y, w, h = (int(v) for v in rects[0])
    assert rect.tolist() == [x, y, w, h] == rough["rect"][0].tolist(), (rect, rects[0])
    assert crop.tobytes() == np.ascontiguousarray(depth[0, y:y + h, x:x + w]).tobytes()
    assert rough["n_model"][0] == np.count_nonzero(depth[0]) > 0
    want = mc.constructed_expected(name)[1][0]
    rows, col = slice(mc.ROOF_ROWS[0], mc.ROOF_ROWS[1] + 1), mc.ROOF_COLUMN
    assert x <= col < x + w and y <= rows.start and rows.stop <= y + h and want[rows, col].all()
    assert np.array_equal(crop[rows.start - y:rows.stop - y, col - x], want[rows, col])        # the ridge: the lower-indexed face's depth
    assert np.array_equal(crop, want[y:y + h, x:x + w]) and np.count_nonzero(want) == rough["n_model"][0]


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------------
def chain_setup():
    """Two frames holding the box a few degrees and millimetres off two views of the table, with clusters at the right place (they converge
    and are kept), at a place beyond the frame (nothing to meet: the pose stays the view's own) and of a view a quarter turn away; a
    third frame that holds nothing, with one cluster (rejected)"""
    tri = rpc.box_mesh()
    base = [rot("y", 20.0) @ rot("x", 35.0), rot("y", -30.0) @ rot("x", 50.0) @ rot("z", 15.0)]
    R = [base[0], rot("z", 3.0) @ base[0], base[1], rot("x", 4.0) @ base[1], rot("x", 90.0) @ base[0]]
    views = rpc.Views(R, [0.5, 0.5, 0.55, 0.55, 0.5])
    scene_views = [(rot("x", 2.0) @ rot("y", -1.5) @ base[0], 0.503), (rot("y", 2.5) @ base[1], 0.546)]
    _, depth, _, rects = render_views(tri, scene_views, W, H, *CAM)
    xy = [(int(r[0]), int(r[1])) for r in rects]
    frames = []
    for f in range(2):
        (x, y), a = xy[f], 2 * f
        rows = [(x + 1, y, 80.0, a, 0), (x - 1, y + 1, 81.0, a + 1, 0), (x, y - 1, 82.0, a, 0),             # the right views at the right place
                (W + 5, 2, 83.0, a, 0), (W + 7, 2, 84.0, a, 0),                                             # ... beyond the frame: nothing to meet
                (x, y, 85.0, 4, 0), (x + 1, y + 1, 86.0, 4, 0)]                                             # a quarter turn away
        frames.append((0, pcc.matches_of(rows), [[0, 1, 2], [3, 4], [5, 6], [1]]))
    frames.append((0, pcc.matches_of([(xy[0][0], xy[0][1], 87.0, 0, 0), (xy[0][0] + 1, xy[0][1], 88.0, 0, 0)]), [[0, 1]]))     # a frame without the object: rejected
    return tri, views, [np.ascontiguousarray(d) for d in depth] + [np.zeros((H, W), np.uint16)], pcc.build_lists(frames)


def test_chain_equals_the_existing_calls_on_the_read_back_crops():
    tri, views, scene, L = chain_setup()
    model = model_of(views, tri=tri)
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    t2 = None
    try:
        t.upload_scene(scene)
        hdr, rough, group, poses, checks, keep = run_hook(t, model, L, rpc.trace_min_of(10.0), room=2)
        n = len(L.clusters)
        assert hdr[0] == n == 9 and rough["status"][:n].tolist() == [OK] * n and hdr[1] == 0 and hdr[5] == n
        assert rough["n_groups"][:n].tolist() == [1] * 9 and rough["n_group_members"][:n].tolist() == [3, 2, 2, 1] * 2 + [2]
        crops = [model.debug_crop(k) for k in range(n)]
        assert all(r.tolist() == rough["rect"][k].tolist() for k, (_, r) in enumerate(crops))
        # the yardstick: the read-back crops as stored templates, one per slot, matched at the mean positions
        t2 = DepthTemplates.from_crops([c for c, _ in crops])
        t2.upload_scene(scene)
        m = pcc.matches_of([(rough["x"][k], rough["y"][k], 90.0, k, 0) for k in range(n)])
        rects = np.asarray([r for _, r in crops], np.int32)
        offsets = [0, 4, 8, 9]
        want_p = t2.refine_poses(m, None, offsets, rects=rects, **PR)
        want_c = t2.verify_poses(m, want_p, None, offsets, rects=rects, **PV)
        want_k = keep_verified(want_c, THRESH)
        for name in POSE_REFINE_DTYPE.names:
            assert poses[name][:n].tobytes() == want_p[name].tobytes(), (name, poses[name][:n], want_p[name])
        assert poses[:n].tobytes() == want_p.tobytes() and checks[:n].tobytes() == want_c.tobytes(), (checks[:n], want_c)
        assert keep[:n].tolist() == want_k.astype(np.uint8).tolist()
        assert hdr[2] == (want_p["status"] != prc.NONE).sum() and hdr[3] == (want_c["status"] == pvc.OK).sum() and hdr[4] == want_k.sum()
        for a in (rough, poses, checks, keep):
            assert (a[n:].view(np.uint8) == CANARY).all()
        # the existing calls alone show both ends
        assert ((want_p["status"] == prc.CONVERGED) & want_k).any() and want_p["status"][8] == prc.NO_OVERLAP and not want_k[8]
        for f in range(2):
            assert want_p["status"][4 * f] == prc.CONVERGED and want_k[4 * f] and want_p["status"][4 * f + 1] == prc.NO_OVERLAP, (f, want_p[4 * f:4 * f + 2])
    finally:
        model.close()
        t.close()
        if t2 is not None:
            t2.close()


# ---- on a real export, on the caller's stream ----------------------------------------------------------------------------------------------------
def export_model():
    views = rpc.Views([rot("y", 4.0 * (k % 10)) @ rot("x", 30.0 + 3.0 * (k // 10)) for k in range(N_T)], [0.5 + 0.02 * (k % 4) for k in range(N_T)])
    cam = (FX, FY, S / 2.0, S / 2.0)
    return views, cam, RoughModel(rpc.box_mesh(), views.pairs(), S, S, *cam, cap_slots=256, max_window=(128, 128))


def test_real_export_equals_the_hook_on_the_same_lists(cfg):  # noqa: F811
    names = ["A", "Z", "B"]
    views, cam, model = export_model()
    kw = dict(scene_camera=cam, max_dist_mm=20.0, max_iterations=4, min_pairs=3, search_radius=1, voxel_mm=8.0, roi_margin=4, threshold_deg=12.0)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            upload_enqueue(cfg, names, stream=stream)
            cfg.t.upload_scene_device(scene_of(cfg, names), stream=stream)
            res = export(cfg, 3, 1, stream=stream, cap_clusters=256, cap_members=1 << 14)
            out = ExportedRoughPoses(256, 1 << 14, stream, torch.cuda.current_device())
            out.member_group.fill_(0x5a5a5a5a)
            assert cfg.t.rough_pose_chain(res, model, THRESH, out=out, **kw) is out and out.stream is stream
            kept = out.clone()
            lists = {k: v.clone() for k, v in res._backing.items()}
            cfg.det.release()
        hdr, rough, group, poses, checks, keep = kept.to_host()
        host = {k: v.cpu().numpy() for k, v in lists.items()}
        n_members = int(host["header"].view(np.uint32)[4])
        assert hdr[0] > 0 and hdr[5] > 0 and (host["frame_info"][:, 6] == 0).all(), (hdr, host["frame_info"])
        assert (rough["n_members"] > 1).any()
        h2, r2, g2, p2, c2, k2 = cfg.t.debug_rough_pose_chain(model, host["header"], host["frame_info"], host["matches"].view(np.uint8).reshape(-1).view(pcc.MATCH_DTYPE),
                                                              host["clusters"].reshape(-1).view(pcc.CLUSTER_DTYPE), host["members"], THRESH, fill=CANARY, **kw)
        n = int(hdr[0])
        assert h2.astype(np.int64).tolist() == hdr.tolist()
        assert r2[:n].tobytes() == rough.tobytes() and g2[:n_members].tobytes() == group[:n_members].tobytes()
        assert p2[:n].tobytes() == poses.tobytes() and c2[:n].tobytes() == checks.tobytes() and k2[:n].astype(bool).tolist() == keep.tolist()
        assert hdr[2] == (poses["status"] != prc.NONE).sum() and hdr[4] == keep.sum()
    finally:
        torch.cuda.synchronize()
        model.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_queued():
    tri, views, scene, L = chain_setup()
    model = model_of(views, tri=tri)
    small = model_of(views, tri=tri, cap_slots=4)
    t = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    empty = DepthTemplates.from_crops([np.full((4, 4), 500, np.uint16)])
    try:
        t.upload_scene(scene)
        stream = torch.cuda.current_stream()
        res = pcc.lists_on_device(L, stream)
        out = t.rough_pose_chain(res, model, THRESH, **KW)
        first = out.to_host()
        hook = run_hook(t, model, L, rpc.trace_min_of(10.0), room=0)
        assert first[1].tobytes() == hook[1].tobytes() and first[3].tobytes() == hook[3].tobytes() and first[4].tobytes() == hook[4].tobytes()
        before = {k: v.clone() for k, v in out._backing.items()}

        def refused(what, change=None, stream_handle=None, templates=None, use_model=None, **kw):
            tt = templates or t
            args = dict(KW)
            args.update(kw)
            d, alive = tt._rough_chain_desc(model, 3, args.pop("keep_thresh", THRESH), 10.0, args.pop("trace_min", None), args.pop("class_index", -1),
                                            args.pop("model_camera"), args.pop("scene_camera"), **args)
            _chain_inputs(d, res)
            _chain_outputs(d, out.NAMES, {k: v.data_ptr() for k, v in out._backing.items()})
            if change:
                change(d, alive)
            with pytest.raises(_lib.LmxError) as e:
                _lib.check(_lib.lib().lmx_rough_pose_chain_on(tt.h, (use_model or model).h, C.byref(d), stream_handle if stream_handle is not None else int(stream.cuda_stream)))
            assert e.value.status == _lib.LMX_ERR_INVALID_ARG and what in str(e.value), (what, str(e.value))

        def field(name, value):
            def change(d, alive):
                setattr(d, name, value)
            return change

        def params_field(which, name, value):
            def change(d, alive):
                setattr(alive[which], name, value)
            return change

        refused("struct_size", field("struct_size", C.sizeof(_lib.RoughChainDesc) - 8))
        refused("struct_size", params_field(0, "struct_size", 8))
        refused("struct_size", params_field(1, "struct_size", 8))
        refused("max_iterations", max_iterations=65)
        refused("voxel_mm", voxel_mm=0.1)
        refused("must not be null", field("header", None))
        refused("must not be null", field("rough", None))
        refused("must not be null", field("member_group", None))
        refused("must not be null", field("keep", None))
        host = np.zeros(64, np.int32)
        refused("members is", field("members", host.ctypes.data))
        refused("member_group is", field("member_group", host.ctypes.data))
        refused("rough must be aligned", field("rough", out._backing["rough"].data_ptr() + 4))
        refused("cap_clusters", field("cap_clusters", 0))
        refused("exceeds the model's cap_slots", use_model=small)
        refused("n_frames", field("n_frames", 0))
        refused("holds 3 frames", field("n_frames", 2))
        refused("keep_thresh", keep_thresh=float("nan"))
        refused("trace_min", trace_min=float("nan"))
        refused("model camera", model_camera=(F + 1.0, F, W / 2.0, H / 2.0))
        rects = np.zeros((1, 4), np.int32)
        refused("rects must be NULL", params_field(0, "rects", rects.ctypes.data))
        refused("rects must be NULL", params_field(1, "rects", rects.ctypes.data))
        refused("no scene", templates=empty)
        hip = C.CDLL("libamdhip64.so")
        hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
        hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        hip.hipGraphDestroy.argtypes = [C.c_void_p]
        side = torch.cuda.Stream()
        graph = C.c_void_p()
        assert hip.hipStreamBeginCapture(side.cuda_stream, 2) == 0                # hipStreamCaptureModeRelaxed
        try:
            refused("captured", stream_handle=int(side.cuda_stream))
        finally:
            assert hip.hipStreamEndCapture(side.cuda_stream, C.byref(graph)) == 0
            if graph.value:
                hip.hipGraphDestroy(graph)
        torch.cuda.synchronize()
        assert all(torch.equal(v, out._backing[k]) for k, v in before.items())      # nothing was written: chain_header included
        again = t.rough_pose_chain(res, model, THRESH, out=out, **KW).to_host()
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(first, again))
        # the model object's own refusals
        for what, kw in (("cap_slots", dict(cap_slots=0)), ("cap_slots", dict(cap_slots=(1 << 16) + 1)), ("window", dict(max_window=(W + 1, 8))),
                         ("window", dict(max_window=(8, 0)))):
            with pytest.raises(_lib.LmxError) as e:
                model_of(views, tri=tri, **kw)
            assert e.value.status == _lib.LMX_ERR_INVALID_ARG and what in str(e.value)
        skew = rpc.Views([np.eye(3) + 1e-5 * np.ones((3, 3))], 0.5)
        with pytest.raises(_lib.LmxError) as e:
            model_of(skew, tri=tri)
        assert "not a rotation" in str(e.value)
    finally:
        torch.cuda.synchronize()
        for o in (model, small, t, empty):
            o.close()
