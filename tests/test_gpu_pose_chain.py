"""lmx_pose_chain_on (csrc/lmx_verify.hip: k_pose_refine_clusters, k_pose_verify_clusters; the decisions: csrc/lmx_pose_chain.hpp) through
DepthTemplates.pose_chain and the hook DepthTemplates.debug_pose_chain.  Nothing here has a tolerance: the yardstick is the host-staged path
that exists without the chain -- cluster_leaders -> refine_poses -> verify_poses -> keep_verified on the same lists and resident scene
(pose_chain_cases.host_staged) -- compared byte for byte.  The crops, scenes and cameras are those of tests/pose_refine_cases.py and
tests/pose_verify_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_chain_cases as pcc
import pose_refine_cases as prc
import pose_verify_cases as pvc
from linemod_pose_estimation_amd import POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE, DepthTemplates, _lib
from linemod_pose_estimation_amd.detector import _chain_inputs, _chain_outputs
from test_gpu_export_clusters import FX, FY, S, cfg, collect, export, scene_of, upload_enqueue  # noqa: F401  (cfg is a fixture)

pytestmark = pytest.mark.gpu

CANARY = 0x5a
THRESH = 0.3
PR = prc.refine_kwargs(prc.make_params(prc.CAM, prc.CAM, max_dist_mm=12.0, max_iterations=6, min_pairs=3, search_radius=1))
PV = pvc.verify_kwargs(pvc.make_params())
KW = dict(PR, **{k: v for k, v in PV.items() if k not in PR})


def the_crops():
    c0, r0 = prc.make_crop(33, 37, (30, 20))
    c1, r1 = prc.make_crop(20, 12, (1, 1), shift=(-1.6, -1.3))
    c3, r3 = prc.make_crop(12, 9, (40, 30), shift=(0.9, 0.6), dz=2.0, drop=0.2, seed=2)
    crops = [c0, c1, np.zeros((0, 0), np.uint16), c3]
    rects = np.asarray([r0 + (33, 37), r1 + (20, 12), (0, 0, 0, 0), r3 + (12, 9)], np.int32)
    return crops, rects


def frame_matches(n, rects, seed, templates=(0, 1, 3)):
    """n matches of class 0 at their template's own place, a pixel off at the most, with distinct similarities below 90"""
    s = (60.0 + np.random.RandomState(seed).permutation(n) * 0.125).astype(np.float32)
    rows = []
    for i in range(n):
        t = templates[i % len(templates)]
        rows.append((int(rects[t, 0]) + i % 3 - 1, int(rects[t, 1]) + (i // 3) % 3 - 1, s[i], t, 0))
    return pcc.matches_of(rows)


@pytest.fixture(scope="module")
def constructed():
    """Three frames, 14 clusters: the object, the resident scene, the lists with everything delivered, and what each cluster is there for."""
    crops, rects = the_crops()
    t = DepthTemplates.from_crops(crops)
    scenes = [prc.make_scene(), prc.make_scene(holes=0.25), pvc.paste(crops[0], (30, 20))]
    t.upload_scene(scenes)
    m0 = frame_matches(93, rects, 1)
    m0["similarity"][[11, 13]] = 95.0                                   # the five-member cluster: positions 1 and 3
    m0["similarity"][[89 - 64, 89 - 69]] = 97.0                         # the 70-member cluster: positions 64 and 69
    m0[90] = (5, 5, 98.0, 2, 0)                                         # a leader whose crop is empty
    m0[91] = (30, 20, 98.0, 0, 1)                                       # a leader of another class
    m0[92] = (prc.SCENE_W + 5, 20, 98.0, 0, 0)                          # a leader that meets no scene pixel
    clusters0 = [[3], [10, 11, 12, 13, 14], list(range(89, 19, -1)), [90, 4], [91, 5], [6, 92], [7, 8], [9, 15, 16], [17], [18, 19]]
    m1 = frame_matches(5, rects, 2)
    m2 = frame_matches(12, rects, 3, templates=(0, 3))
    clusters2 = [[0, 1], [2], [3, 4, 5], [6, 7, 8, 9, 10, 11]]
    L = pcc.build_lists([(0, m0, clusters0), (1, m1, []), (0, m2, clusters2)])
    assert len(L.clusters) == 14
    yield t, rects, L
    t.close()


def run_hook(t, L, rects, cap_clusters=None, **kw):
    args = dict(KW, class_index=0, rects=rects)
    args.update(kw)
    return t.debug_pose_chain(L.header, L.frame_info, L.matches, L.clusters, L.members, THRESH, cap_clusters=cap_clusters, fill=CANARY, **args)


def check_against_host(got, want, n_live, n_slots, flags, what):
    """got: the hook's five outputs; want: host_staged's {slot: ...} for the processed slots"""
    hdr, leaders, poses, checks, keep = got
    for k in range(n_slots):
        one = (leaders[k:k + 1], poses[k:k + 1], checks[k:k + 1], keep[k:k + 1])
        if k >= n_live:                                                  # not written: every byte still the canary
            assert all((a.view(np.uint8) == CANARY).all() for a in one), (what, k)
        elif k in want:
            lead, p, c, kept = want[k]
            assert int(leaders[k]) == lead, (what, k)
            for name in POSE_REFINE_DTYPE.names:
                assert poses[name][k].tobytes() == p[name][0].tobytes(), (what, k, name, poses[name][k], p[name][0])
            assert poses[k:k + 1].tobytes() == p.tobytes() and checks[k:k + 1].tobytes() == c.tobytes(), (what, k, checks[k], c)
            assert int(keep[k]) == int(kept), (what, k)
        else:                                                            # dead below n_live
            assert int(leaders[k]) == -1 and not poses[k:k + 1].view(np.uint8).any() and not checks[k:k + 1].view(np.uint8).any() and keep[k] == 0, (what, k)
    p = np.concatenate([v[1] for v in want.values()]) if want else np.zeros(0, POSE_REFINE_DTYPE)
    c = np.concatenate([v[2] for v in want.values()]) if want else np.zeros(0, POSE_VERIFY_DTYPE)
    kept = sum(int(v[3]) for v in want.values())
    assert hdr.tolist() == [n_live, flags, int((p["status"] != prc.NONE).sum()), int((c["status"] == pvc.OK).sum()), kept, 0, 0, 0], (what, hdr)
    return p, c


def test_constructed_lists_equal_the_host_staged_path(constructed):
    t, rects, L = constructed
    want = pcc.host_staged(t, L, {0, 2}, 0, PR, PV, THRESH, rects)
    p, c = check_against_host(run_hook(t, L, rects), want, 14, 14, 0, "everything fits")
    roomy = L.copy()                                                    # room for two clusters more than the export delivered: not written
    roomy.clusters = np.concatenate([L.clusters, L.clusters[:2]])
    check_against_host(run_hook(t, roomy, rects), want, 14, 16, 0, "room to spare")
    # what the clusters were built for
    lead = [want[k][0] for k in range(14)]
    assert lead[:6] == [3, 11, 25, 90, 91, 92] and want[2][0] == L.members[L.clusters[2]["member_begin"] + 64]
    assert p["status"][3] == p["status"][4] == prc.NONE and p["status"][5] == prc.NO_OVERLAP and c["status"][5] != pvc.NONE
    assert {int(v) for v in p["status"]} >= {prc.NONE, prc.NO_OVERLAP} and {int(v) for v in p["status"]} & {prc.CONVERGED, prc.MAX_ITERATIONS}
    assert {int(v) for v in c["status"]} >= {pvc.NONE, pvc.OK}
    assert 0 < sum(int(v[3]) for v in want.values()) < 14
    # the export that cuts inside the last frame reports status 8 for it; and the same cut by this call's own capacity alone
    cut = L.copy()
    cut.frame_info[2, 6] = 8
    first = {k: v for k, v in want.items() if k < 10}
    for lists, what in ((cut, "status 8"), (L, "this call's cap_clusters")):
        got = run_hook(t, lists, rects, cap_clusters=12)
        check_against_host(got, first, 12, 14, pcc.FLAG_CUT, what)
    # the host-staged records did not change under the chain's launches
    again = pcc.host_staged(t, L, {0, 2}, 0, PR, PV, THRESH, rects)
    assert all(again[k][1].tobytes() == want[k][1].tobytes() and again[k][2].tobytes() == want[k][2].tobytes() for k in want)


def test_class_base_rebases_the_template_ids():
    crops, rects = the_crops()
    a, b = DepthTemplates.from_crops([crops[0], crops[1]]), DepthTemplates.from_crops([crops[3], crops[0]])
    a.append(b)
    b.close()
    joined = np.concatenate([rects[[0, 1]], rects[[3, 0]]])
    base = [0, 2, 4]
    try:
        scenes = [prc.make_scene(), pvc.paste(crops[0], (30, 20))]
        a.upload_scene(scenes)
        rows = []
        for i in range(16):
            cls, tid = i % 2, (i // 2) % 2
            r = joined[base[cls] + tid]
            rows.append((int(r[0]) + i % 3 - 1, int(r[1]), 70.0 + i, tid, cls))
        m = pcc.matches_of(rows)
        L = pcc.build_lists([(0, m, [[0, 1, 2], [3], [4, 5]]), (0, m[::-1].copy(), [[0, 1], [2, 3, 4], [15]])])
        want = pcc.host_staged(a, L, {0, 1}, -1, PR, PV, THRESH, joined, class_base=base)
        got = run_hook(a, L, joined, class_index=5, class_base=base)    # class_index is ignored with class_base
        p, c = check_against_host(got, want, 6, 6, 0, "class_base")
        assert {int(L.matches[v[0]]["class_index"]) for v in want.values()} == {0, 1} and (p["status"] != prc.NONE).all() and (c["status"] == pvc.OK).any()
        # without class_base class 1's ids name other crops: the records differ
        other = run_hook(a, L, joined, class_index=-1)
        assert other[2].tobytes() != got[2].tobytes()
    finally:
        a.close()


POSE_KW = dict(model_camera=(FX, FY, S / 2.0, S / 2.0), scene_camera=(FX, FY, S / 2.0, S / 2.0), max_dist_mm=20.0, max_iterations=4, min_pairs=3, search_radius=1)
VERIFY_KW = dict(voxel_mm=8.0, roi_margin=4)


def test_end_to_end_without_the_host_in_between(cfg):  # noqa: F811
    names = ["A", "Z", "B"]
    rects = cfg.rects
    cams = dict(model_camera=POSE_KW["model_camera"], scene_camera=POSE_KW["scene_camera"])
    want = {}
    for alt in (False, True):      # the yardstick: the same enqueue collected, its clusters through the host-staged functions against the same scene
        upload_enqueue(cfg, names)
        cfg.t.upload_scene_device(scene_of(cfg, names, alt))
        per_frame = []
        for f, (m, _, _, cl, _, mem) in enumerate(collect(cfg, 3, 1)):
            lead = pcc.cluster_leaders(cl, mem, m) if len(cl) else np.zeros(0, np.int64)
            lm = m[lead]
            offs = [0] * (f + 1) + [len(lm)] * (3 - f)
            p = cfg.t.refine_poses(lm, None, offs, rects=rects, **POSE_KW)
            c = cfg.t.verify_poses(lm, p, None, offs, rects=rects, **cams, **VERIFY_KW)
            per_frame.append((lead, p, c, pcc.keep_verified(c, THRESH)))
        want[alt] = per_frame
    # the chain twice on one stream with nothing in between but the stream's order: enqueue, scene, export, poses; a copy of the first
    # round's results (the second round writes the same tensors); release, which waits for the export that read the slot and not for the
    # poses; the other scene -- uploaded while the first round's kernels may still read the old one --, and the second round.  The results
    # are read once, at the end.
    stream = torch.cuda.Stream()
    res = poses = None
    kept = []
    with torch.cuda.stream(stream):
        for alt in (False, True):
            upload_enqueue(cfg, names, stream=stream)
            cfg.t.upload_scene_device(scene_of(cfg, names, alt), stream=stream)
            res = export(cfg, 3, 1, stream=stream, out=res)
            poses = cfg.t.pose_chain(res, THRESH, rects=rects, out=poses, **POSE_KW, **VERIFY_KW)
            assert poses.stream is stream
            kept.append((poses.clone(), res.frame_info.clone()))
            cfg.det.release()
    for alt, (got, info) in zip((False, True), kept):
        hdr, leaders, p, c, keep = got.to_host()
        info = info.cpu().numpy()
        assert hdr[0] == sum(len(w[0]) for w in want[alt]) > 0 and hdr[1] == 0 and (info[:, 6] == 0).all(), (hdr, info)
        for f, (lead, wp, wc, wk) in enumerate(want[alt]):
            cb, cc, mb = int(info[f, 2]), int(info[f, 3]), int(info[f, 0])
            assert cc == len(lead)
            assert np.array_equal(leaders[cb:cb + cc], lead + mb), (alt, f)
            assert p[cb:cb + cc].tobytes() == wp.tobytes() and c[cb:cb + cc].tobytes() == wc.tobytes() and np.array_equal(keep[cb:cb + cc], wk), (alt, f)
        assert hdr[2] == (p["status"] != prc.NONE).sum() > 0 and hdr[3] == (c["status"] == pvc.OK).sum() and hdr[4] == keep.sum()
    assert kept[0][0].to_host()[2].tobytes() != kept[1][0].to_host()[2].tobytes()        # the two scenes gave different poses


def test_refusals_come_before_anything_is_queued(constructed):
    t, rects, L = constructed
    stream = torch.cuda.current_stream()
    res = pcc.lists_on_device(L, stream)
    want = pcc.host_staged(t, L, {0, 2}, 0, PR, PV, THRESH, rects)
    out = t.pose_chain(res, THRESH, class_index=0, rects=rects, **KW)
    first = out.to_host()
    assert [int(v) for v in first[1]] == [want[k][0] for k in range(14)] and first[2].tobytes() == b"".join(want[k][1].tobytes() for k in range(14))
    assert first[3].tobytes() == b"".join(want[k][2].tobytes() for k in range(14)) and first[4].tolist() == [want[k][3] for k in range(14)]
    before = {k: v.clone() for k, v in out._backing.items()}
    t.set_profiling(True)

    def refused(what, change=None, stream_handle=None, templates=None, **kw):
        tt = templates or t
        args = dict(KW, class_index=0, rects=rects if templates is None else None)
        args.update(kw)
        d, alive = tt._pose_chain_desc(3, args.pop("keep_thresh", THRESH), args.pop("class_index"), args.pop("class_base", None), **args)
        _chain_inputs(d, res)
        _chain_outputs(d, out.NAMES, {k: v.data_ptr() for k, v in out._backing.items()})
        if change:
            change(d, alive)
        with pytest.raises(_lib.LmxError) as e:
            _lib.check(_lib.lib().lmx_pose_chain_on(tt.h, C.byref(d), stream_handle if stream_handle is not None else int(stream.cuda_stream)))
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG and what in str(e.value), (what, str(e.value))

    def field(name, value):
        def change(d, alive):
            setattr(d, name, value)
        return change

    def params_size(which):
        def change(d, alive):
            alive[which].struct_size += 8
        return change

    refused("struct_size", field("struct_size", C.sizeof(_lib.PoseChainDesc) - 8))
    refused("struct_size", params_size(0))
    refused("struct_size", params_size(1))
    refused("max_iterations", max_iterations=65)
    refused("voxel_mm", voxel_mm=0.1)
    refused("must not be null", field("header", None))
    refused("must not be null", field("keep", None))
    host = np.zeros(64, np.int32)
    refused("members is", field("members", host.ctypes.data))
    pinned = torch.zeros(64, dtype=torch.int32).pin_memory()
    refused("leaders is", field("leaders", pinned.data_ptr()))
    refused("clusters must be aligned", field("clusters", res._backing["clusters"].data_ptr() + 4))
    refused("poses must be aligned", field("poses", out._backing["poses"].data_ptr() + 4))
    refused("cap_clusters", field("cap_clusters", 0))
    refused("cap_clusters", field("cap_clusters", (1 << 20) + 1))
    refused("n_frames", field("n_frames", 0))
    refused("holds 3 frames", field("n_frames", 2))
    refused("class_base ends", class_base=[0, 2, 5])
    refused("class_base", class_base=[1, 2, 4])
    refused("keep_thresh", keep_thresh=float("nan"))
    empty = DepthTemplates.from_crops(the_crops()[0])
    try:
        refused("no scene", templates=empty)
    finally:
        empty.close()
    # a stream that is being captured: the capture is begun and ended here, nothing is replayed
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
    times = t.kernel_times()
    t.set_profiling(False)
    assert times["k_pose_refine_clusters"][1] == 0 and times["k_pose_verify_clusters"][1] == 0      # nothing was launched for any of them
    torch.cuda.synchronize()
    assert all(torch.equal(v, out._backing[k]) for k, v in before.items())                          # and nothing was written
    # the object still completes a valid call, into the same tensors
    again = t.pose_chain(res, THRESH, class_index=0, rects=rects, out=out, **KW).to_host()
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(first, again))
