"""The scene filter beside plane stages and a schedule in one launch (csrc/lmx_verify.hip: pose_scene_on hands the pose kernels the filtered
copy, plane_normals_on the normals of the RAW scene; both validity flags are dropped from seven places), against the composition of three
CPU headers of tests/pose_settings_cases.py -- no device value is part of it, and tests/test_pose_settings_cases_host.py shows that it
differs from the two ways of mixing the scenes up.  Every pose path, state sequences on one object, the raw-scene rule of the cluster
scores, and the launch counts.  Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import normal_verify_cases as nvc
import pose_chain_cases as pcc
import pose_refine_cases as prc
import pose_settings_cases as psx
import pose_verify_cases as pvc
import rough_pose_cases as rpc
import second_trip_cases as stc
from linemod_pose_estimation_amd import POSE_REFINE_DTYPE, DepthTemplates, _lib
from pose_settings_cases import CAM, H, KW, PR, PV, THRESH, W
from test_gpu_rough_pose import model_of

pytestmark = pytest.mark.gpu

CANARY = 0x5a


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return stc.Hosts(tmp_path_factory.mktemp("pose_settings_gpu"))


@pytest.fixture(scope="module")
def S():
    return psx.setup()


def templates(S):
    t = DepthTemplates.from_mesh(S.tri, S.views.pairs(), W, H, *CAM)
    for i, c in enumerate(S.crops):                                       # the composition's crops are the object's
        assert t.rect(i) == tuple(int(v) for v in S.rects[i]) and np.array_equal(t.crop(i), c), i
    return t


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.names:
        for k in got.dtype.names:
            assert got[k].tobytes() == want[k].tobytes(), (what, k, np.nonzero([got[k][i].tobytes() != want[k][i].tobytes() for i in range(len(got))])[0][:4], got[k][:2], want[k][:2])
    assert got.tobytes() == want.tobytes(), what


def refine_resident(t, S):
    return t.refine_poses(S.L.matches, None, S.offsets, **PR)


def test_every_pose_path_equals_the_composition(S, hosts):
    st = psx.Settings()
    poses, sums, planes, checks = psx.compose(hosts, S, st, S.raw)
    m, offs = S.L.matches, S.offsets
    t = templates(S)
    model = model_of(S.views, tri=S.tri)
    try:
        st.apply(t)
        t.upload_scene(S.raw)
        same(refine_resident(t, S), poses, "refine_poses, resident")
        same(t.verify_poses(m, poses, None, offs, **PV), checks, "verify_poses, resident")
        # the chains on the resident scene
        leaders, cp, cc, ck = psx.compose_chain(hosts, S, st, S.raw)
        n = len(S.L.clusters)
        hdr, gl, gp, gc, gk = t.debug_pose_chain(S.L.header, S.L.frame_info, m, S.L.clusters, S.L.members, THRESH, fill=CANARY, class_index=0, **KW)
        assert [int(v) for v in gl] == [int(v) for v in leaders]
        same(gp, cp, "debug_pose_chain poses")
        same(gc, cc, "debug_pose_chain checks")
        assert gk.tolist() == ck.astype(np.uint8).tolist()
        assert hdr.tolist() == [n, 0, int((cp["status"] != prc.NONE).sum()), int((cc["status"] == pvc.OK).sum()), int(ck.sum()), 0, 0, 0] and ck.any()
        out = t.pose_chain(pcc.lists_on_device(S.L, torch.cuda.current_stream()), THRESH, class_index=0, **KW).to_host()
        assert out[0].tolist() == hdr.tolist() and [int(v) for v in out[1][:n]] == [int(v) for v in leaders]
        same(out[2][:n], cp, "pose_chain poses")
        same(out[3][:n], cc, "pose_chain checks")
        assert out[4][:n].tolist() == gk.tolist()
        rough = psx.rough_records(hosts, S)
        rp, rc, rk = psx.compose_rough_chain(hosts, S, st, S.raw, rough)
        rhdr, rrec, _, gp, gc, gk = t.debug_rough_pose_chain(model, S.L.header, S.L.frame_info, m, S.L.clusters, S.L.members, THRESH, trace_min=rpc.trace_min_of(psx.TRACE_DEG),
                                                             fill=CANARY, **KW)
        for k, (rec, crop, rect, _) in enumerate(rough):                  # the rough stage reads no scene: its records and renders are the header's and the host rasteriser's
            assert rrec[k:k + 1].tobytes()[:128] == rec.tobytes()[:128] and rrec["rect"][k].tolist() == rect.tolist() and np.array_equal(model.debug_crop(k)[0], crop), k
        same(gp, rp, "debug_rough_pose_chain poses")
        same(gc, rc, "debug_rough_pose_chain checks")
        assert gk.tolist() == rk.astype(np.uint8).tolist() and rhdr[0] == n and rhdr[2] == (rp["status"] != prc.NONE).sum() and rhdr[4] == rk.sum() > 0
        # staged frames: the filter and the normals are made of the frames of the call
        same(t.refine_poses(m, S.raw, offs, **PR), poses, "refine_poses, staged")
        same(t.verify_poses(m, poses, S.raw, offs, **PV), checks, "verify_poses, staged")
        steps = 0
        for i in (0, 1, 5, 7, 12, 14):
            f = int(np.searchsorted(offs, i, side="right")) - 1
            rec, s17, s29 = t.debug_pose_refine_plane_sums(S.raw[f], m[i:i + 1], **PR)
            same(np.asarray([rec]), poses[i:i + 1], ("plane sums hook: record", i))
            assert np.array_equal(s17, sums[i]), ("the 17 sums", i, np.nonzero((s17 != sums[i]).any(1))[0][:3])
            assert np.array_equal(s29, planes[i]), ("the 29 plane sums", i, np.nonzero((s29 != planes[i]).any(1))[0][:3])
            steps += int(planes[i][:, 0].astype(bool).sum())
        assert steps > 10
        # a staged call forgets the resident scene: the next resident call is refused until a new upload
        with pytest.raises(_lib.LmxError) as e:
            refine_resident(t, S)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "no scene is uploaded" in str(e.value)
        t.upload_scene(S.raw)
        same(refine_resident(t, S), poses, "refine_poses, resident again")
    finally:
        model.close()
        t.close()


def test_state_sequence_on_one_object(S, hosts):
    """Each step against the composition for the scene and the settings then in force: a stale filtered copy or stale normals give the
    bytes of the step before (tests/test_pose_settings_cases_host.py: every step's composition differs from its neighbour's)."""
    st = psx.Settings()
    t = templates(S)
    never = templates(S)
    try:
        st.but(scene_filter=None).apply(t, order=("normals", "stages", "shifts"))
        t.upload_scene(S.raw)
        steps = []

        def step(what, settings, frames, got):
            want = psx.compose(hosts, S, settings, frames)[0]
            same(got, want, what)
            assert not steps or steps[-1].tobytes() != want.tobytes(), what        # the step changed what is expected
            steps.append(want)

        step("plane refine, normals computed, no filter", st.but(scene_filter=None), S.raw, refine_resident(t, S))
        t.set_scene_filter(*st.scene_filter, camera=CAM)
        step("the filter set on the resident scene", st, S.raw, refine_resident(t, S))
        t.upload_scene(S.other)
        step("a new upload", st, S.other, refine_resident(t, S))
        st2 = st.but(scene_filter=(2, 9, 0.5))
        t.set_scene_filter(*st2.scene_filter, camera=CAM)
        step("the filter set with other parameters", st2, S.other, refine_resident(t, S))
        st3 = st2.but(normals=(psx.F, psx.F, 20, 640))
        t.enable_normals(*st3.normals)
        step("normals enabled with other thresholds", st3, S.other, refine_resident(t, S))
        step("a staged call with other frames", st3, S.raw, t.refine_poses(S.L.matches, S.raw, S.offsets, **PR))
        with pytest.raises(_lib.LmxError) as e:                                       # the staged call took the scene's place: what the library does today
            refine_resident(t, S)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "no scene is uploaded" in str(e.value)
        t.upload_scene(S.other)
        step("a resident call after a new upload", st3, S.other, refine_resident(t, S))
        same(t.verify_poses(S.L.matches, steps[-1], None, S.offsets, **PV), psx.compose(hosts, S, st3, S.other)[3], "verify_poses at the end of the sequence")
        # everything off again: the bytes of an object that never had the settings, which are the point-to-point header's on the raw frames
        t.set_refine_plane(None)
        t.set_refine_schedule(None)
        t.set_scene_filter(None)
        never.upload_scene(S.other)
        plain = refine_resident(never, S)
        same(refine_resident(t, S), plain, "the settings cleared")
        frame_of = np.repeat(np.arange(3), np.diff(S.offsets))
        for i, mm in enumerate(S.L.matches):
            tid = int(mm["template_id"])
            want, _ = prc.host_refine(hosts.pose("pr"), psx.P, S.crops[tid], S.rects[tid, :2], S.other[frame_of[i]], mm["x"], mm["y"], POSE_REFINE_DTYPE)
            same(plain[i:i + 1], want, ("never set", i))
        assert plain.tobytes() != steps[-1].tobytes()
        # the same settings in the other order: the filter first, the normals (and the shifts that need them) last
        st3.apply(never, order=("scene_filter", "stages", "normals", "shifts"))
        same(refine_resident(never, S), steps[-1], "set in the other order")
    finally:
        t.close()
        never.close()


def test_cluster_scores_and_stored_normals_keep_the_raw_scene(S, hosts):
    st = psx.Settings()
    t, twin = templates(S), templates(S)
    try:
        st.apply(t)
        st.but(scene_filter=None).apply(twin, order=("normals", "stages", "shifts"))
        for x in (t, twin):
            x.upload_scene(S.raw)
        a, b = refine_resident(t, S), refine_resident(twin, S)                        # the filtered copy exists now
        assert a.tobytes() != b.tobytes()
        assert (t.debug_scene_filtered(0)[0] != S.raw[0]).any()
        for f in range(3):
            want = nvc.host_map(hosts.nv, S.raw[f], *st.normals)
            assert np.array_equal(t.debug_scene_normals(f), want) and np.array_equal(twin.debug_scene_normals(f), want), f
        same(refine_resident(t, S), a, "after the hooks")
        m, offs = S.L.matches, S.offsets
        d, (dd, nd) = t.diff(S.raw, m, offs), t.normal_diff(S.raw, m, offs)
        wd, (wdd, wnd) = twin.diff(S.raw, m, offs), twin.normal_diff(S.raw, m, offs)
        assert d.tobytes() == wd.tobytes() == dd.tobytes() == wdd.tobytes() and nd.tobytes() == wnd.tobytes()
        assert d["n_valid"].any() and nd["n_normal"].any()
        filtered = [psx.scenes_for(hosts, st, [r])[0][0] for r in S.raw]
        assert twin.diff(filtered, m, offs).tobytes() != wd.tobytes()                 # the filtered frames would have given other sums
    finally:
        t.close()
        twin.close()


def test_one_filter_and_one_normal_map_launch_per_scene(S):
    st = psx.Settings()
    t = templates(S)
    try:
        st.apply(t)
        t.set_profiling(True)
        t.upload_scene(S.raw)
        first = refine_resident(t, S)
        second = refine_resident(t, S)
        t.verify_poses(S.L.matches, first, None, S.offsets, **PV)
        times = t.kernel_times()
        t.set_profiling(False)
        assert first.tobytes() == second.tobytes()
        assert times["k_scene_filter_score"][1] == 1 and times["k_scene_filter_apply"][1] == 1 and times["k_normal_map_frames"][1] == 1, times
        assert times["k_pose_refine"][1] == 2 and times["k_pose_verify"][1] == 1, times
    finally:
        t.close()
