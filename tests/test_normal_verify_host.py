"""The normal term of a match without a device: the shared header (csrc/lmx_normal_verify.hpp, built with plain g++ from
tests/cpp/normal_verify_host.cpp) against the numpy restatement of tests/normal_verify_cases.py, the analytic plane angles, the angle
table, lmx_match_value, the same file's main() under AddressSanitizer + UBSan as a child process, and the argument checks of every new
entry point that can be reached without a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import normal_verify_cases as nvc
from conftest import has_gpu
from linemod_pose_estimation_amd import _lib
from linemod_pose_estimation_amd import DEPTH_DIFF_DTYPE, MATCH_DTYPE, NORMAL_DIFF_DTYPE, DepthTemplates, normal_angle_table, normal_values

SRC, FLAGS = nvc.HOST_SRC, nvc.HOST_FLAGS


@pytest.fixture(scope="module")
def nv(tmp_path_factory):
    return nvc.build_host_lib(tmp_path_factory.mktemp("nvhost"))


host_map = nvc.host_map


def host_diff(lib, crop, crop_n, scene, scene_n, x, y, table):
    out = np.zeros(5, np.int64)
    h, w = crop.shape
    lib.nv_host_diff(crop.ctypes.data, crop_n.ctypes.data, w, h, w, scene.ctypes.data, scene_n.ctypes.data, scene.shape[1], scene.shape[0], scene.shape[1],
                     int(x), int(y), table.ctypes.data, out.ctypes.data)
    return out


def host_diff_vectors(lib, crop, crop_n, scene, scene_n, x, y, table):
    """The same match the way the kernel walks it: whole vectors over rows padded with zeros to the pitch, depths and normals alike."""
    out = np.zeros(5, np.int64)
    h, w = crop.shape
    pitch = (w + 7) // 8 * 8
    crop_p, crop_np = nvc.padded(crop, pitch), nvc.padded(crop_n, pitch)
    lib.nv_host_diff_vectors(crop_p.ctypes.data, crop_np.ctypes.data, h, pitch, scene.ctypes.data, scene_n.ctypes.data, scene.shape[1], scene.shape[0],
                             scene.shape[1], int(x), int(y), table.ctypes.data, out.ctypes.data)
    return out


def test_table():
    t = normal_angle_table()
    assert t.shape == (16385,) and t[0] == 0 and t[8192] == 1047198 and t[16384] == 3141593
    assert (np.diff(t.astype(np.int64)) >= 0).all()
    assert np.abs(t.astype(np.int64) - nvc.np_angle_table().astype(np.int64)).max() <= 1
    assert _lib.lib().lmx_normal_angle_table(None) == _lib.LMX_ERR_INVALID_ARG


def test_header_table_is_the_librarys(nv):
    t = np.zeros(16385, np.uint32)
    nv.nv_host_table(t.ctypes.data)
    assert np.array_equal(t, normal_angle_table())


def test_normal_map_equals_the_restatement(nv):
    n_valid = n_invalid = 0
    for name, img in nvc.constructed_images():
        got = host_map(nv, img)
        assert np.array_equal(got, nvc.np_normal_map(img)), name
        wide = np.full((img.shape[0], img.shape[1] + 3), 1234, np.uint16)      # the same image as a strided view
        wide[:, :img.shape[1]] = img
        assert np.array_equal(host_map(nv, wide[:, :img.shape[1]]), got), name
        n_valid += int(got[..., 3].sum())
        n_invalid += int((got[..., 3] == 0).sum())
        assert not got[got[..., 3] == 0].any()                   # an invalid normal is all zeros
    assert n_valid > 5000 and n_invalid > 1000
    # other parameters: thresholds that change which taps count, unequal focal lengths
    img = dict(nvc.constructed_images())["noise around the difference threshold"]
    for kw in (dict(fx=500.0, fy=1100.0), dict(diff_t=1), dict(diff_t=20, dist_t=810), dict(diff_t=65535, dist_t=65535)):
        a = host_map(nv, img, **kw)
        b = nvc.np_normal_map(img, kw.get("fx", nvc.FX), kw.get("fy", nvc.FY), kw.get("diff_t", nvc.DIFF_T), kw.get("dist_t", nvc.DIST_T))
        assert np.array_equal(a, b), kw


def test_threshold_cases(nv):
    imgs = dict(nvc.constructed_images())
    assert host_map(nv, imgs["at distance_threshold - 1"])[..., 3].all()
    assert not host_map(nv, imgs["at distance_threshold"]).any()
    assert not host_map(nv, imgs["no measurement"]).any()
    # slope 9: every tap counts and the normal is the plane's; slope 10: the x taps are gone, what is left is a singular system (the
    # three taps of the centre column cannot tell the x slope): det = 0, hence s = 0 and no normal where no other tap helps
    n9 = host_map(nv, imgs["plane a=9 b=0"])
    n10 = host_map(nv, imgs["plane a=10 b=0"])
    assert n9[..., 3].all() and not n10[5:-5, 5:-5, 3].any()
    d = imgs["plane a=9 b=0"][9, 11].astype(np.float64)
    want = np.asarray([nvc.FX * 9, 0.0, -d]) / np.linalg.norm([nvc.FX * 9, 0.0, d]) * 16384
    assert np.abs(n9[9, 11, :3] - want).max() <= 1.0


def test_analytic_plane_angles(nv):
    """Plane pairs: the table's angle against the analytic one.  Bound: each stored component is off by at most 0.5 / 16384 (rintf) plus
    float rounding, so the chord of two normals by less than 2 * sqrt(3) * 0.5 / 16384 = 1.74 / 16384, its half -- the index -- by less
    than 0.87, and rintf adds 0.5: the true half chord lies within 2 index steps, the analytic angle between table[i - 2] and
    table[i + 2] (one more microradian for the table's own rounding)."""
    table = normal_angle_table().astype(np.int64)
    pairs = [((0, 0), (0, 0)), ((1, 0), (0, 1)), ((3, -2), (-4, 5)), ((9, 0), (0, -9)), ((9, 9), (-4, 5)), ((9, 0), (9, 0)), ((0, 0), (9, 9))]
    checked = 0
    for (a0, b0), (a1, b1) in pairs:
        p0, p1 = nvc.plane(23, 19, 700, a0, b0), nvc.plane(23, 19, 700, a1, b1)
        n0, n1 = host_map(nv, p0), host_map(nv, p1)
        assert n0[..., 3].all() and n1[..., 3].all()
        idx = nvc.np_angle_index(n0, n1)
        for (y, x) in ((9, 11), (0, 0), (18, 22), (3, 20)):
            assert nv.nv_host_angle_index(int(nvc.packed(n0)[y, x]), int(nvc.packed(n1)[y, x])) == idx[y, x]
        want = nvc.plane_angle(nvc.FX, nvc.FY, a0, b0, p0, a1, b1, p1) * 1e6
        lo, hi = table[np.maximum(idx - 2, 0)] - 1, table[np.minimum(idx + 2, 16384)] + 1
        assert ((lo <= want) & (want <= hi)).all(), ((a0, b0), (a1, b1))
        checked += idx.size
    up, down = nvc.opposed_planes()
    nu, nd = host_map(nv, up), host_map(nv, down)
    idx = nvc.np_angle_index(nu, nd)
    want = nvc.plane_angle(nvc.FX, nvc.FY, 9, 0, up, -9, 0, down) * 1e6
    assert ((table[np.maximum(idx - 2, 0)] - 1 <= want) & (want <= table[np.minimum(idx + 2, 16384)] + 1)).all()
    assert want.max() > np.radians(169.0) * 1e6 and abs(np.degrees(2 * np.arctan(800 * 9 / 100.0)) - 178.4) < 0.1
    assert checked > 2000


def _pairs():
    imgs = nvc.constructed_images()
    by = dict(imgs)
    out = [(by["plane with holes"], by["noise around the difference threshold"]), (by["noise around the difference threshold"], by["plane with holes"]),
           (by["steps across both thresholds"], by["plane a=3 b=-2"]), (by["any values"], by["any values"]), (by["scene 12x13"], by["scene 70x37"]),
           (by["scene 65x11"], by["scene 64x37"]), (by["plane a=9 b=0"], by["plane a=0 b=-9"])]
    # rows of 64, 65 and 138 vectors: up to one, two and three trips of a wave's 64 lanes along a row
    crops, _, scene, _, _ = nvc.wide()
    assert sorted(c.shape[::-1] for c in crops) == [(505, 1), (505, 5), (513, 1), (513, 5), (1100, 5)]
    out += [(c, scene) for c in crops] + [(crops[-1][2:3], scene)]                   # and 1100 x 1
    return out


def _positions(w, h, W, H):
    m = 2 ** 31
    return [(0, 0), (1, 2), (-1, 0), (0, -1), (-1, -1), (W - w, H - h), (W - w + 1, 0), (0, H - h + 1), (W - 1, H - 1), (-(w // 2), H - 1 - h // 2),
            (W, 0), (0, H), (-w, 0), (0, -h), (m - 1, 0), (0, m - 1), (-m, -m), (m - 1 - w, m - 1 - h)]


def test_match_sums_and_value_equal_the_restatement(nv):
    table = normal_angle_table()
    n = with_normals = without = 0
    for crop, scene in _pairs():
        crop, scene = np.ascontiguousarray(crop), np.ascontiguousarray(scene)
        cn, sn = host_map(nv, crop), host_map(nv, scene)
        assert np.array_equal(cn, nvc.np_normal_map(crop)) and np.array_equal(sn, nvc.np_normal_map(scene))
        for x, y in _positions(crop.shape[1], crop.shape[0], scene.shape[1], scene.shape[0]):
            got = host_diff(nv, crop, cn, scene, sn, x, y, table).tolist()
            want = list(nvc.np_normal_diff(crop, cn, scene, sn, x, y, table))
            assert got == want, (crop.shape, scene.shape, x, y)
            assert host_diff_vectors(nv, crop, cn, scene, sn, x, y, table).tolist() == want, (crop.shape, scene.shape, x, y)
            for no_value in (-np.inf, -7.5):
                v = nv.nv_host_value(got[0], got[1], got[3], got[4], no_value)
                assert v == nvc.np_value(got[0], got[1], got[3], got[4], no_value)
            n += 1
            with_normals += got[4] > 0
            without += got[4] == 0 and got[1] > 0
    assert n > 100 and with_normals > 30 and without > 0


def test_identical_data_gives_zero(nv):
    table = normal_angle_table()
    for name, img in nvc.constructed_images():
        img = np.ascontiguousarray(img)
        n = host_map(nv, img)
        got = host_diff(nv, img, n, img, n, 0, 0, table).tolist()
        assert got[0] == 0 and got[3] == 0 and got[4] == int(n[..., 3].sum()), name
    up, _ = nvc.opposed_planes()
    n = host_map(nv, up)
    assert host_diff(nv, up, n, up, n, 0, 0, table).tolist()[4] == 64 * 64


def test_opposed_planes_pass_2_to_32(nv):
    table = normal_angle_table()
    up, down = nvc.opposed_planes()
    got = host_diff(nv, up, host_map(nv, up), down, host_map(nv, down), 0, 0, table).tolist()
    want = nvc.np_normal_diff(up, nvc.np_normal_map(up), down, nvc.np_normal_map(down), 0, 0, table)
    assert got == list(want) and got[4] == 4096 and got[3] > 2 ** 32


def test_match_value_and_normal_values(nv):
    L = _lib.lib()
    d = np.zeros(5, DEPTH_DIFF_DTYPE)
    n = np.zeros(5, NORMAL_DIFF_DTYPE)
    d["sum_abs_mm"], d["n_valid"] = [0, 7000, 4311612928, 5, 0], [10, 7, 65792, 3, 0]
    n["sum_angle_urad"], n["n_normal"] = [0, 3141593, 12432966656, 0, 9], [10, 2, 4096, 0, 4]
    v = normal_values(d, n)
    assert v[0] == 0.0 and v[1] == -(1.0 + 3141593 / 2e6) and v[3] == -np.inf and v[4] == -np.inf
    for i in range(5):
        for no_value in (-np.inf, -3.25):
            dd = _lib.DepthDiff(int(d["sum_abs_mm"][i]), int(d["n_valid"][i]), 0)
            nd = _lib.NormalDiff(int(n["sum_angle_urad"][i]), int(n["n_normal"][i]), 0)
            got = L.lmx_match_value(C.byref(dd), C.byref(nd), no_value)
            want = nv.nv_host_value(int(d["sum_abs_mm"][i]), int(d["n_valid"][i]), int(n["sum_angle_urad"][i]), int(n["n_normal"][i]), no_value)
            assert got == want and (no_value != -np.inf or got == v[i])
    dd, nd = _lib.DepthDiff(1, 1, 1), _lib.NormalDiff(1, 1, 0)
    assert L.lmx_match_value(None, C.byref(nd), -2.0) == -2.0 and L.lmx_match_value(C.byref(dd), None, -2.0) == -2.0
    with pytest.raises(ValueError):
        normal_values(d, n[:3])


def test_cases_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "normal_verify_host")
    subprocess.check_call(["g++"] + FLAGS + san + [SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "normal_verify_host ok" in res.stdout


# ---- argument checks (no device needed up to the point where LMX_ERR_NO_DEVICE is the answer) ------------------------------------------

def _image(a, channels=1, elem_size=2):
    return _lib.Image(a.ctypes.data, a.shape[0], a.shape[1], channels, elem_size, a.strides[0])


def test_enable_normals_and_accessor_argument_checks():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16), np.zeros((0, 0), np.uint16)])   # two empty templates: no device touched
    buf = np.zeros(8, np.int16)
    assert L.lmx_depth_templates_get_normals(t.h, 0, buf.ctypes.data) == INV and b"enable_normals" in L.lmx_last_error()
    bytes_before = t.device_bytes

    def enable(h=t.h, fx=800.0, fy=800.0, diff=50, dist=2000, null=False):
        p = _lib.NormalParams(fx, fy, diff, dist)
        return L.lmx_depth_templates_enable_normals(h, None if null else C.byref(p))

    assert enable(h=None) == INV and enable(null=True) == INV and b"null" in L.lmx_last_error()
    for kw in (dict(fx=0.0), dict(fy=-1.0), dict(fx=float("nan")), dict(fy=float("inf")), dict(fx=2e6), dict(diff=0), dict(dist=0), dict(dist=-5)):
        assert enable(**kw) == INV, kw
    assert t.device_bytes == bytes_before
    assert enable() == _lib.LMX_OK and enable() == _lib.LMX_OK and enable(diff=40) == _lib.LMX_OK     # no pixel: no device
    assert t.device_bytes == bytes_before + 2 * 8                # one address per template, no crop element
    assert L.lmx_depth_templates_get_normals(None, 0, buf.ctypes.data) == INV
    assert L.lmx_depth_templates_get_normals(t.h, 2, buf.ctypes.data) == INV and b"id 2" in L.lmx_last_error()
    assert L.lmx_depth_templates_get_normals(t.h, -1, buf.ctypes.data) == INV
    assert t.normals(1).shape == (0, 0, 4)
    assert L.lmx_debug_scene_normals(None, 0, buf.ctypes.data) == INV and L.lmx_debug_scene_normals(t.h, 0, None) == INV
    assert L.lmx_debug_scene_normals(t.h, 0, buf.ctypes.data) == INV and b"no scene" in L.lmx_last_error()
    t.close()
    if not has_gpu():
        t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16)])
        L.lmx_depth_templates_free(t.h)
        t.h = None
        h = C.c_void_p()
        crop = np.ones((3, 5), np.uint16)
        assert L.lmx_depth_templates_from_crops(0, (C.c_void_p * 1)(crop.ctypes.data), (C.c_int32 * 2)(5, 3), 1, C.byref(h)) == _lib.LMX_ERR_NO_DEVICE


def test_normal_diff_matches_argument_checks():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16), np.zeros((0, 0), np.uint16)])
    d0, d1 = np.ones((12, 16), np.uint16), np.ones((12, 16), np.uint16)
    m = np.zeros(3, MATCH_DTYPE)
    dd = np.full(3, 7, DEPTH_DIFF_DTYPE)
    out = np.full(3, 7, NORMAL_DIFF_DTYPE)

    def diff(h=t.h, imgs=(d0, d1), images=None, nf=2, matches=m, offsets=(0, 1, 3), cls=-1, d=dd, o=out):
        arr = images if images is not None else ((_lib.Image * len(imgs))(*[_image(a) for a in imgs]) if imgs is not None else None)
        offs = (C.c_size_t * len(offsets))(*offsets) if offsets is not None else None
        return L.lmx_normal_diff_matches(h, arr, nf, matches.ctypes.data if matches is not None else None, offs, cls,
                                         d.ctypes.data if d is not None else None, o.ctypes.data if o is not None else None)

    assert diff() == INV and b"enable_normals" in L.lmx_last_error() and b"lmx_normal_diff_matches" in L.lmx_last_error()
    t.enable_normals(800.0, 800.0)
    assert diff(h=None) == INV and b"null" in L.lmx_last_error()
    assert diff(imgs=None) == INV and diff(offsets=None) == INV and diff(matches=None) == INV and diff(o=None) == INV
    assert diff(nf=-1) == INV and b"n_frames" in L.lmx_last_error()
    assert diff(offsets=(1, 1, 3)) == INV and diff(offsets=(0, 2, 1)) == INV and b"offsets" in L.lmx_last_error()
    bgr = np.ones((12, 16, 3), np.uint8)
    two = (_lib.Image * 2)(_image(d0), _lib.Image(bgr.ctypes.data, 12, 16, 3, 1, bgr.strides[0]))
    assert diff(images=two) == _lib.LMX_ERR_SHAPE and b"image 1" in L.lmx_last_error() and b"one channel of 2 bytes" in L.lmx_last_error()
    assert diff(imgs=(d0, np.ones((12, 17), np.uint16))) == _lib.LMX_ERR_SHAPE and b"image 1 is 17 x 12" in L.lmx_last_error()
    assert diff(images=(_lib.Image * 2)(_image(d0), _lib.Image(None, 12, 16, 1, 2, 32))) == INV
    bad = m.copy()
    bad["template_id"][2] = 2
    assert diff(matches=bad) == INV and b"match 2" in L.lmx_last_error() and b"template_id 2" in L.lmx_last_error()
    bad["class_index"][2] = 4
    bad["class_index"][:2] = 1
    assert diff(matches=bad, cls=0) == _lib.LMX_OK and not out.view(np.uint8).any() and not dd.view(np.uint8).any()   # nothing selected: zeros, no device
    out[:] = 7
    assert diff(matches=bad, cls=0, d=None) == _lib.LMX_OK and not out.view(np.uint8).any()                            # ddiffs may be NULL
    assert diff(nf=0, imgs=None, offsets=None, matches=None, o=None) == _lib.LMX_OK
    assert diff(offsets=(0, 0, 0), matches=None, o=None) == _lib.LMX_OK
    if not has_gpu():
        assert diff() == _lib.LMX_ERR_NO_DEVICE
    t.close()


def test_collect_clusters_depth_normal_argument_checks():
    L = _lib.lib()
    INV = _lib.LMX_ERR_INVALID_ARG
    t = DepthTemplates.from_crops([np.zeros((0, 0), np.uint16)])
    mo, co = (C.c_size_t * 2)(), (C.c_size_t * 2)()
    args = (1, t.h, -1)
    assert L.lmx_ctx_collect_clusters_depth_normal(None, *args, -1.0, None, 0, mo, None, None, None, 0, co, None, 0) == INV and b"null" in L.lmx_last_error()
    assert L.lmx_ctx_collect_clusters_depth_normal(None, *args, float("nan"), None, 0, mo, None, None, None, 0, co, None, 0) == INV
    assert b"not a number" in L.lmx_last_error()
    t.close()
