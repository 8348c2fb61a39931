"""The scene's depth outlier filter without a device: the shared header (csrc/lmx_scene_filter.hpp, built with plain g++ from
tests/cpp/scene_filter_host.cpp) against the brute-force numpy restatement of tests/scene_filter_cases.py in every byte of the filtered map
and of the record; the routes the small frames were built for; the three constructed scenes, where exactly the planted pixels go; the
corner rule at k = 16; the header's own refusals and the setter's, which need no device; tests/cpp/scene_filter_main.cpp under
AddressSanitizer + UBSan as a child process."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import scene_filter_cases as sfc
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd import DepthTemplates


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sfc.build_host(tmp_path_factory.mktemp("sfhost"))


@pytest.fixture(scope="module")
def results(host):
    """Every small frame through the restatement and the header, equal in every byte -> {name: (scene, record, q, state)}."""
    out = {}
    for name, scene, cam, r, k, mul in sfc.small_cases():
        want, rec, q, state = sfc.np_filter(scene, cam, r, k, mul)
        rc, got, info = sfc.host_filter(host, scene, cam, r, k, mul)
        assert rc == 0, name
        assert want.tobytes() == got.tobytes(), (name, np.argwhere(want != got)[:5])
        assert sfc.record_array(rec).tobytes() == info.tobytes(), (name, rec, info)
        out[name] = (scene, rec, q, state)
    return out


def test_record_layout(host):
    assert sfc.INFO_DTYPE.itemsize == 56 == host.sf_host_info_bytes() == C.sizeof(_lib.SceneFilterInfo)
    assert C.sizeof(_lib.SceneFilterParams) == 56
    assert [f[0] for f in _lib.SceneFilterInfo._fields_] == list(sfc.INFO_FIELDS) == list(DepthTemplates.SCENE_FILTER_INFO_FIELDS)


def test_header_equals_the_numpy_restatement(results):
    assert len(results) == len(sfc.small_cases())
    for name, (scene, rec, q, state) in results.items():
        assert rec["n_valid"] == int((scene != 0).sum()) == rec["n_sparse"] + rec["n_scored"], name
        assert 0 <= rec["n_removed"] <= rec["n_scored"], name


def test_every_route_occurs(results):
    def rec(name):
        return results[name][1]

    assert rec("1x1") == dict(n_valid=1, n_sparse=1, n_scored=0, n_removed=0, sum_q=0, sum_qq=0, threshold=2.0 ** 20)
    assert rec("3x3_r1_k3")["n_scored"] == 9 and rec("5x4_r3")["n_scored"] == 20                     # a corner of a 3 x 3 frame has exactly 3 neighbours
    assert rec("all_zero") == dict(n_valid=0, n_sparse=0, n_scored=0, n_removed=0, sum_q=0, sum_qq=0, threshold=2.0 ** 20)
    one = rec("one_scored")
    assert one["n_scored"] == 1 and one["n_sparse"] == 8 and one["n_removed"] == 0 and one["threshold"] == 2.0 ** 20 and one["sum_q"] > 0    # n < 2: kept
    eq = rec("all_q_equal")
    assert eq["n_scored"] == 30 and eq["sum_q"] == 30 * 2048 and eq["sum_qq"] == 30 * 2048 ** 2 and eq["threshold"] == 2048.0 and eq["n_removed"] == 0   # var = 0
    assert rec("r7_k224")["n_scored"] == 6 and rec("r7_k224")["n_sparse"] == 17 * 16 - 6 and rec("r7_k1")["n_sparse"] == 0
    # ties: the k-th distance is one of several equal ones, on either side of the step from 32 to 45
    assert set(np.unique(results["ties_k2"][2])) == {(2 * 32 << 16) // (2 * 1024)}
    q6, st6 = results["ties_k6"][2], results["ties_k6"][3]
    assert set(np.unique(q6[st6 == sfc.SCORED])) == {((4 * 32 + 2 * 45) << 16) // (6 * 1024)} and (st6 == sfc.SPARSE).sum() == 2 * 6 + 2 * 5 - 4
    # the 2^14 bound alone decides whether the centre has its eighth neighbour
    assert rec("bound_at")["n_scored"] == 1 and rec("bound_beyond")["n_scored"] == 0 and rec("bound_beyond")["n_sparse"] == 9
    # 1 mm among 900 mm: its score is clamped; the two pixels of 65535 mm have one neighbour each and k = 2
    scene, r, q, st = results["clamp"]
    assert q[1, 1] == sfc.MAX_Q and st[1, 1] == sfc.SCORED and (st[scene == 65535] == sfc.SPARSE).all() and r["n_removed"] >= 1
    # a camera that throws all but one pixel far off: those have no point
    assert rec("far")["n_sparse"] == rec("far")["n_valid"] == 30
    base, zero, wide = rec("41x37"), rec("mul_0"), rec("mul_16")
    assert 0 < base["n_removed"] < zero["n_removed"] and wide["n_removed"] <= base["n_removed"] and base["sum_qq"] == zero["sum_qq"] == wide["sum_qq"]
    assert zero["threshold"] < base["threshold"] < wide["threshold"] and 0 < rec("33x9")["n_removed"] < rec("33x9")["n_scored"]
    routes = {"sparse": 0, "clamped": 0, "removed": 0, "kept": 0}
    for name, (scene, r, q, st) in results.items():
        routes["sparse"] += r["n_sparse"]
        routes["clamped"] += int(((st == sfc.SCORED) & (q == sfc.MAX_Q)).sum())
        routes["removed"] += r["n_removed"]
        routes["kept"] += r["n_scored"] - r["n_removed"]
    assert all(v > 0 for v in routes.values()), routes


@pytest.mark.parametrize("index", range(3))
def test_constructed_scenes_lose_exactly_the_planted_pixels(host, index):
    name, scene, planted = sfc.constructed_scenes()[index]
    cam = sfc.scene_camera(scene)
    rc, got, info = sfc.host_filter(host, scene, cam)
    want, rec, q, state = sfc.np_filter(scene, cam)
    assert rc == 0 and got.tobytes() == want.tobytes() and info.tobytes() == sfc.record_array(rec).tobytes(), name
    expect = scene.copy()
    for p in planted:
        expect[p] = 0
    assert np.array_equal(got, expect), (name, np.argwhere(got != expect))
    assert rec["n_sparse"] == 0 and rec["n_removed"] == len(planted) and rec["n_scored"] == int((scene != 0).sum()), (name, rec)
    print(name, "threshold", rec["threshold"], "planted q", [int(q[p]) for p in planted])


def test_corner_rule_at_k_16(host):
    """(r + 1)^2 - 1 = 15 is what a right-angle corner pixel keeps of its own surface: with k = 16 the box's corners go, and the image's
    corners, which have 15 neighbours in all, are sparse."""
    name, scene, planted = sfc.constructed_scenes()[2]
    cam = sfc.scene_camera(scene)
    rc, got, info = sfc.host_filter(host, scene, cam, k=16)
    want, rec, q, state = sfc.np_filter(scene, cam, k=16)
    assert rc == 0 and got.tobytes() == want.tobytes() and info.tobytes() == sfc.record_array(rec).tobytes()
    H, W = scene.shape
    image_corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    box_corners = [(10, 12), (10, 35), (29, 12), (29, 35)]
    expect = scene.copy()
    for p in planted + image_corners + box_corners:
        expect[p] = 0
    assert np.array_equal(got, expect), np.argwhere(got != expect)
    assert rec["n_sparse"] == 4 and all(state[p] == sfc.SPARSE for p in image_corners) and all(state[p] == sfc.SCORED for p in box_corners)
    assert rec["n_removed"] == len(planted) + 4


def test_header_refuses_parameters_out_of_range(host):
    s = np.full((4, 5), 700, np.uint16)
    nan, inf = float("nan"), float("inf")

    def rc(cam=(570.0, 570.0, 2.5, 2.0), r=3, k=15, mul=1.0):
        return sfc.host_filter(host, s, cam, r, k, mul)[0]

    assert rc() == 0 and rc(r=1, k=8) == 0 and rc(r=7, k=224) == 0 and rc(mul=0.0) == 0 and rc(mul=16.0) == 0
    for bad in (dict(r=0), dict(r=8), dict(r=-1), dict(k=0), dict(k=49), dict(r=1, k=9), dict(r=7, k=225), dict(mul=-0.001), dict(mul=16.001), dict(mul=nan), dict(mul=inf),
                dict(cam=(0.0, 570.0, 2.5, 2.0)), dict(cam=(570.0, -1.0, 2.5, 2.0)), dict(cam=(570.0, 570.0, nan, 2.0)), dict(cam=(570.0, 570.0, 2.5, inf)),
                dict(cam=(570.0, 570.0, 0.0, 2.0)), dict(cam=(inf, 570.0, 2.5, 2.0))):
        assert rc(**bad) == 1, bad


def test_setter_refusals_need_no_device():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16)])   # an empty template: no device touched
    p = _lib.SceneFilterParams()
    assert L.lmx_scene_filter_defaults(None) == INV
    assert L.lmx_scene_filter_defaults(C.byref(p)) == _lib.LMX_OK
    assert (p.struct_size, p.radius, p.k, p.reserved, p.stddev_mul, p.fx, p.fy, p.cx, p.cy) == (56, 3, 15, 0, 1.0, 0.0, 0.0, 0.0, 0.0)
    assert L.lmx_depth_templates_set_scene_filter(None, C.byref(p)) == INV and b"null" in L.lmx_last_error()
    assert L.lmx_depth_templates_set_scene_filter(t.h, C.byref(p)) == INV and b"camera" in L.lmx_last_error()     # the defaults carry no camera
    buf = np.zeros((4, 4), np.uint16)
    assert L.lmx_debug_scene_filtered(t.h, 0, buf.ctypes.data, None) == INV and b"set_scene_filter first" in L.lmx_last_error()
    t.set_scene_filter(camera=(570.0, 570.0, 320.0, 240.0))
    assert L.lmx_debug_scene_filtered(t.h, 0, buf.ctypes.data, None) == INV and b"no scene" in L.lmx_last_error()   # the setting is in place
    assert L.lmx_debug_scene_filtered(None, 0, buf.ctypes.data, None) == INV and L.lmx_debug_scene_filtered(t.h, 0, None, None) == INV
    nan, inf = float("nan"), float("inf")

    def refused(**kw):
        q = _lib.SceneFilterParams()
        L.lmx_scene_filter_defaults(C.byref(q))
        q.fx, q.fy, q.cx, q.cy = 570.0, 570.0, 320.0, 240.0
        for k, v in kw.items():
            setattr(q, k, v)
        return L.lmx_depth_templates_set_scene_filter(t.h, C.byref(q))

    assert refused() == _lib.LMX_OK
    assert refused(struct_size=48) == INV and b"struct_size" in L.lmx_last_error()
    assert refused(reserved=1) == INV and b"reserved" in L.lmx_last_error()
    for bad in (dict(radius=0), dict(radius=8), dict(k=0), dict(k=49), dict(radius=1, k=9), dict(stddev_mul=-1.0), dict(stddev_mul=16.5), dict(stddev_mul=nan),
                dict(fx=0.0), dict(fy=-570.0), dict(cx=nan), dict(cy=inf), dict(fx=inf)):
        assert refused(**bad) == INV, bad
    assert b"camera" in L.lmx_last_error()
    assert refused(radius=7, k=224, stddev_mul=16.0) == _lib.LMX_OK and refused(radius=1, k=1, stddev_mul=0.0) == _lib.LMX_OK
    # a refusal leaves the previous setting in place: the hook still gets past "set_scene_filter first"
    assert refused(radius=9) == INV
    assert L.lmx_debug_scene_filtered(t.h, 0, buf.ctypes.data, None) == INV and b"no scene" in L.lmx_last_error()
    # off again; the Python front end's own refusal
    t.set_scene_filter(None)
    assert L.lmx_debug_scene_filtered(t.h, 0, buf.ctypes.data, None) == INV and b"set_scene_filter first" in L.lmx_last_error()
    with pytest.raises(ValueError):
        t.set_scene_filter()
    with pytest.raises(ValueError):
        t.set_scene_filter(None, k=9, camera=(570.0, 570.0, 320.0, 240.0))        # None switches off and takes nothing else
    with pytest.raises(_lib.LmxError) as e:
        t.set_scene_filter(radius=2, k=25, camera=(570.0, 570.0, 320.0, 240.0))
    assert e.value.status == INV and "k must lie" in str(e.value)
    with pytest.raises(ValueError):
        t.debug_scene_filtered(0)
    t.close()


def test_hostile_frames_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "scene_filter_main")
    subprocess.check_call(["g++"] + sfc.HOST_FLAGS + san + [sfc.MAIN_SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "scene_filter_main ok" in res.stdout
