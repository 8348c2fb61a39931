"""The mesh rasteriser's device header on the CPU (tests/cpp/mesh_raster_host.cpp: linemod_pose_estimation_amd/csrc/lmx_mesh_raster.hpp
compiled with LMX_MR_HOST, -ffp-contract=off) against meshsynth.render_view (meshraster.c), every byte of gray, depth, mask and rect; and
the argument checks of the two entry points built on it (lmx_mesh_render, lmx_bank_train_mesh).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
from conftest import ROOT, has_gpu
from linemod_pose_estimation_amd import _lib, meshsynth as ms, NativeBank

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")


@pytest.fixture(scope="module")
def mr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mrhost") / "libmrhost.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "mesh_raster_host.cpp")])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.mr_host_render.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, C.c_int, vp, vp, vp, vp]
    return lib


def host_render(lib, tri, cam, views, fill=0x5a):
    tri = np.ascontiguousarray(tri, np.float64)
    n, H, W = len(views), cam["height"], cam["width"]
    pv = mc.pack_views(views)
    light = np.asarray(mc.LIGHT, np.float64)
    gray = np.full((n, H, W), fill, np.uint8)
    depth = np.full((n, H, W), fill, np.uint16)
    mask = np.full((n, H, W), fill, np.uint8)
    rects = np.full((n, 4), -7, np.int32)
    rc = lib.mr_host_render(tri.ctypes.data, len(tri), W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], light.ctypes.data, pv.ctypes.data, n,
                            gray.ctypes.data, depth.ctypes.data, mask.ctypes.data, rects.ctypes.data)
    return rc, gray, depth, mask, rects


CASES = mc.cases()
CONSTRUCTED = mc.constructed_cases()
CONSTRUCTED_NAMES = {c[0] for c in CONSTRUCTED}


@pytest.mark.parametrize("case", CASES + CONSTRUCTED, ids=[c[0] for c in CASES + CONSTRUCTED])
def test_header_equals_meshraster_c(mr, case):
    name, tri, cam, views = case
    rc, gray, depth, mask, rects = host_render(mr, tri, cam, views)
    assert rc == -1
    eg, ed, em, er = mc.constructed_expected(name) if name in CONSTRUCTED_NAMES else mc.expected(tri, cam, views)
    assert np.array_equal(rects, er), (rects, er)
    assert np.array_equal(mask, em), np.argwhere(mask != em)[:5]
    assert np.array_equal(depth, ed), np.argwhere(depth != ed)[:5]
    assert np.array_equal(gray, eg), np.argwhere(gray != eg)[:5]
    if name in CONSTRUCTED_NAMES:     # their conditions: test_constructed_cases_are_what_they_claim
        return
    covered = (em > 0).reshape(len(views), -1).sum(1)
    H, W = cam["height"], cam["width"]
    if name.endswith("outside"):
        assert covered.max() == 0 and not rects.any() and not gray.any() and not depth.any()
    else:
        assert covered.min() > 100    # the comparison is not about empty images (the smallest: cpu_binary at a third of the focal length)
    touches = {"left": er[0][0] == 0, "right": er[0][0] + er[0][2] == W, "top": er[0][1] == 0, "bottom": er[0][1] + er[0][3] == H}
    for side, hit in touches.items():
        if name == "chip_cut_" + side:
            assert hit and covered[0] > 3000 and er[0][2] * er[0][3] > 0
    if name == "chip_ties_degenerates":   # duplicates and degenerates change nothing: equal to the plain mesh
        pg, pd, pm, pr = mc.expected(ms.load_mesh("memoryChip2"), cam, views)
        assert np.array_equal(gray, pg) and np.array_equal(depth, pd) and np.array_equal(mask, pm) and np.array_equal(rects, pr)


def test_case_list_is_what_it_claims():
    names = [c[0] for c in CASES]
    assert len(CASES[0][3]) >= 60 and len(CASES[1][3]) >= 60 and len(set(names)) == len(names)
    tri = CASES[-1][1]
    assert len(tri) > len(ms.load_mesh("memoryChip2")) + 150


def _case(name):
    return next(c for c in CONSTRUCTED if c[0] == name)


def _alone(case, index):
    """meshsynth's render of one triangle of a case (first view) -> gray, depth, mask [H, W]."""
    _, tri, cam, views = case
    g, d, m, _ = mc.expected(tri[index:index + 1], cam, views[:1])
    return g[0], d[0], m[0]


def _lattice_claims():
    on_edge_total = 0
    for case in CONSTRUCTED:
        name, tri, cam, views = case
        if not name.startswith("lattice_"):
            continue
        eg, ed, em, er = mc.constructed_expected(name)
        winner, z, on_edge = mc.numpy_render(tri, cam, views[0])
        covered = winner >= 0
        assert covered.sum() >= 1, name
        # the rule restated in numpy gives meshraster.c's coverage and depth
        assert np.array_equal(covered, em[0] > 0), name
        assert np.array_equal(np.where(covered, np.clip(np.rint(np.where(covered, z, 0.0) * 1000.0), 0, 65535), 0).astype(np.uint16), ed[0]), name
        print("%s: covered %d, winner's centre exactly on an edge or vertex %d" % (name, covered.sum(), (on_edge & covered).sum()))
        on_edge_total += int((on_edge & covered).sum())
    assert on_edge_total >= 50
    assert {(c[2]["width"], c[2]["height"]) for c in CONSTRUCTED if c[0].startswith("lattice_")} == set(mc.LATTICE_FRAMES)


def _roof_claims():
    x, (y0, y1) = mc.ROOF_COLUMN, mc.ROOF_ROWS
    ridge = np.zeros((mc.ROOF_CAM["height"], mc.ROOF_CAM["width"]), bool)
    ridge[y0:y1 + 1, x] = True
    ab, ba = mc.constructed_expected("roof_ab"), mc.constructed_expected("roof_ba")
    left, right = _alone(_case("roof_ab"), 0), _alone(_case("roof_ab"), 1)
    g_left, g_right = int(left[0][18, 5]), int(right[0][18, 30])
    assert g_left != g_right and left[2][18, 5] and right[2][18, 30]
    for first, second, tag in ((ab, ba, ""), ) + tuple((mc.constructed_expected("roof_ab_after_%d" % n), mc.constructed_expected("roof_ba_after_%d" % n), n) for n in mc.ROOF_FILLERS):
        differ = (first[0][0] != second[0][0]) | (first[1][0] != second[1][0]) | (first[2][0] != second[2][0])
        print("roof %s: the two orders differ in %d pixels, %d of them on the ridge" % (tag, differ.sum(), (differ & ridge).sum()))
        assert (differ & ridge).sum() >= 8 and not (differ & ~ridge).any()
        assert np.array_equal(differ, ridge)                      # every ridge pixel is an exact tie: the lower index shows
        assert np.all(first[0][0][ridge] == g_left) and np.all(second[0][0][ridge] == g_right)
        assert np.array_equal(first[1][0][ridge], second[1][0][ridge])      # equal z: equal depth
        assert np.array_equal(first[3], second[3])
    for n in mc.ROOF_FILLERS:
        name, tri, cam, views = _case("roof_ab_after_%d" % n)
        hits = mc.tile_hits(tri, cam, views[0])
        assert len(tri) == n + 2 and hits[:, :n].all()       # the filler hits every tile: in the roof's tiles the tie is decided at slots n, n + 1
        assert (hits[:, n] & hits[:, n + 1])[0:15:3].all()     # the ridge's tiles (column 0, rows 0 .. 4) stage both faces
        got = mc.constructed_expected(name)
        on_roof = ab[2][0] > 0
        assert np.array_equal(got[0][0][on_roof], ab[0][0][on_roof]) and np.array_equal(got[1][0][on_roof], ab[1][0][on_roof])
        assert got[1][0][~on_roof].min() >= 8000 and got[2][0].all()          # the filler lies behind and shows everywhere else


def _fan_claims():
    x, (y0, y1) = mc.ROOF_COLUMN, mc.ROOF_ROWS
    firsts = []
    for k in range(mc.FAN_ORDERS):
        case = _case("roof_fan_%d_order_%d" % (mc.FAN_N, k))
        name, tri, cam, views = case
        eg, ed, em, er = mc.constructed_expected(name)
        hits = mc.tile_hits(tri, cam, views[0])
        assert len(tri) == mc.FAN_N and hits[0:15:3].all()          # the ridge's tiles stage every face: chunks of 256, 256 and 88 hits
        # every face alone gives the ridge the same depth (an exact tie), and its own gray
        grays = np.empty(len(tri), np.int64)
        for t in range(len(tri)):
            g, d, m = _alone(case, t)
            assert m[y0:y1 + 1, x].all() and np.array_equal(d[y0:y1 + 1, x], ed[0][y0:y1 + 1, x]), (name, t)
            grays[t] = g[18, x]
            assert np.all(g[y0:y1 + 1, x] == grays[t])
        assert np.all(eg[0][y0:y1 + 1, x] == grays[0])            # the lowest index shows
        print("%s: %d grays among the faces, %d faces share face 0's" % (name, len(np.unique(grays)), (grays == grays[0]).sum() - 1))
        # (planes through one line are a one-parameter family: their grays span 88 .. 105 here, no more)
        assert len(np.unique(grays)) >= 15 and (grays != grays[0]).sum() >= 0.75 * (len(tri) - 1)
        firsts.append(grays[0])
    assert len(set(firsts)) == mc.FAN_ORDERS                      # the orders put faces of different gray first


def _stack_claims():
    info = mc.constructed_info()["stack"]
    names = [c[0] for c in CONSTRUCTED if c[0].startswith("stack_")]
    assert sorted(names) == sorted(info) and len(names) == 1 + 3 * (len(mc.STACK_N) - 1) + 1
    for name in names:
        case = _case(name)
        _, tri, cam, views = case
        eg, ed, em, er = mc.constructed_expected(name)
        assert em.all()
        for y0, y1, index in info[name]["winners"]:
            g, d, m = _alone(case, index)
            assert m[y0:y1].all() and np.array_equal(eg[0][y0:y1], g[y0:y1]) and np.array_equal(ed[0][y0:y1], d[y0:y1]), (name, index)
        if info[name]["runner_up"] is not None:      # the next plane behind the winner would show another gray and another depth everywhere
            g, d, m = _alone(case, info[name]["runner_up"])
            assert np.all(g != eg[0]) and np.all(d > ed[0]), name
        hits = mc.tile_hits(tri, cam, views[0])
        assert hits.shape[0] == 3 * 6
        if len(tri) >= mc.CHUNK:
            assert hits[:, :mc.CHUNK].all(), name        # every tile stages a full chunk 0
        if name != "stack_600_hole":
            assert hits.all()
    _, tri, cam, views = _case("stack_600_hole")
    hits = mc.tile_hits(tri, cam, views[0])
    assert hits[:, 512:].all() and len(tri) == 600
    assert not hits[:9, 256:512].any()                                     # tile rows 0 .. 2: chunk 1 has no hits
    for tile in range(9, 18):
        waves = [hits[tile, 256 + 64 * w:320 + 64 * w] for w in range(4)]
        assert waves[0].all() and waves[2].all()
        if tile == 17:                                                      # the corner tile: chunk 1 is full too
            assert waves[1].all() and waves[3].all()
        else:                                                               # 64 hits next to none
            assert not waves[1].any() and not waves[3].any()
    g599, g447 = _alone(_case("stack_600_hole"), 599)[0], _alone(_case("stack_600_hole"), 447)[0]
    assert g599[0, 0] != g447[30, 0]


def _sliver_and_huge_claims():
    name, tri, cam, views = _case("slivers_150x117")
    eg, ed, em, er = mc.constructed_expected(name)
    covered = int((em > 0).sum())
    print("slivers: %d triangles cover %d pixels with %d grays" % (len(tri), covered, len(np.unique(eg[em > 0]))))
    assert len(tri) == 3000 and 100 <= covered <= 5000 and len(np.unique(eg[em > 0])) >= 20
    u, v, _ = mc.project(tri, cam, views[0])
    length = np.hypot(u[:, 1] - u[:, 0], v[:, 1] - v[:, 0])
    width = np.abs((u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (v[:, 1] - v[:, 0]) * (u[:, 2] - u[:, 0])) / length
    assert length.min() >= 5 - 1e-6 and length.max() <= 200 + 1e-6 and width.max() <= 0.3 + 1e-6 and width.min() < 1e-8
    name, tri, cam, views = _case("huge_150x117")
    eg, ed, em, er = mc.constructed_expected(name)
    print("huge: %d of %d pixels covered" % ((em > 0).sum(), em.size))
    assert len(tri) == 400 and (em > 0).sum() * 2 >= em.size
    u, v, _ = mc.project(tri, cam, views[0])
    reach = np.maximum(np.abs(u), np.abs(v)).max(1)
    assert reach.max() <= 1.0001e8 and (reach > 1e7).sum() >= 20 and reach.min() < 1e3


def _clamped_claims():
    name, tri, cam, views = _case("clamped_out_65x17")
    plain = mc.constructed_info()["clamped_plain"]
    assert len(tri) == len(plain) + 4 * len(mc.CLAMP_OFFSETS)
    for a, b in zip(mc.constructed_expected(name), mc.expected(plain, cam, views)):
        assert np.array_equal(a, b)
    out = mc.clamped_out(np.random.RandomState(0), cam)
    assert all(any(np.array_equal(t, o) for t in tri) for o in out)
    x0, x1, y0, y1, drawn = mc.clamped_boxes(out, cam, views[0])
    empty = (x1 < x0) | (y1 < y0)
    print("clamped out: %d boxes empty after the clamp, %d not" % (empty.sum(), (~empty).sum()))
    assert drawn.all() and empty.sum() >= 8 and (~empty).sum() >= 4
    assert not (mc.expected(out, cam, views)[2] > 0).any()        # alone they cover nothing


def _depth_claims():
    seen = {}
    for label, Z in mc.DEPTH_PLANES:
        eg, ed, em, er = mc.constructed_expected("depth_mm_" + label)
        assert em.all()
        seen[label] = sorted(set(ed.ravel().tolist()))
        print("depth plane %s mm (1000 Z = %.17g): %s" % (label, Z * 1000.0, seen[label]))
    assert 1.0125 * 1000.0 == 1012.5 and seen["1012.5"] == [1012]                # a tie, to even
    assert 2.0005 * 1000.0 > 2000.5 and seen["2000.5"] == [2001]                 # the double next to 2.0005 lies above the tie
    assert 2.0025 * 1000.0 == 2002.5 and set(seen["2002.5"]) <= {2002, 2003} and 2002 in seen["2002.5"]
    assert 0.0105 * 1000.0 == 10.5 and set(seen["10.5"]) <= {10, 11}
    assert seen["65534"] == [65534]
    assert 65.5345 * 1000.0 < 65534.5 and set(seen["65534.5"]) <= {65534, 65535} and 65534 in seen["65534.5"]
    assert seen["65535.5"] == [65535] and seen["70000"] == [65535]


def _batch_claims():
    name, tri, cam, views = _case("batch_chip_75x41")
    H, W = cam["height"], cam["width"]
    eg, ed, em, er = mc.constructed_expected(name)
    covered = (em > 0).reshape(len(views), -1).sum(1)
    print("batch (chip): covered %s, rects %s, centre depth %s" % (covered.tolist(), er.tolist(), ed[:, H // 2, W // 2].tolist()))
    assert len(views) == 7 and (W, H) == (75, 41)
    for i in (0, 2, 5, 6):
        assert covered[i] > 100
    for i in (1, 3):
        assert not er[i].any() and not eg[i].any() and not ed[i].any() and not em[i].any()
        x0, x1, y0, y1, drawn = mc.clamped_boxes(tri, cam, views[i])
        assert drawn.any() and np.all((x1 < x0) | (y1 < y0))        # drawn triangles, every box empty after the clamp
    x, y, w, h = er[4]
    assert covered[4] >= 1 and x >= 64 and y >= 40 and w >= 1 and h >= 1
    hits = mc.tile_hits(tri, cam, views[4]).any(1)
    assert hits[17] and not hits[:14].any() and not hits[15:17].any()    # boxes reach one row above what they cover: the 11x1 corner tile and the one above it
    assert em[5, H // 2, W // 2] == 255 and ed[5, H // 2, W // 2] > 0
    assert em[6, H // 2, W // 2] == 0 and ed[6, H // 2, W // 2] == 0

    name, tri, cam, views = _case("batch_plane_75x41")
    eg, ed, em, er = mc.constructed_expected(name)
    covered = (em > 0).reshape(len(views), -1).sum(1)
    print("batch (plane): covered %s" % covered.tolist())
    assert len(views) == 7
    for i in (0, 2, 4, 6):
        assert covered[i] > 100
    for i in (1, 3, 5):
        assert not er[i].any() and not eg[i].any() and not ed[i].any() and not em[i].any()
    assert mc.clamped_boxes(tri, cam, views[1])[4].any()
    for i in (3, 5):                                               # edge-on: v is the same double for every vertex, every area is exactly 0
        u, v, Z = mc.project(tri, cam, views[i])
        assert np.all(v == cam["cy"]) and Z.min() > 0.01 and not mc.clamped_boxes(tri, cam, views[i])[4].any()


def _corner_claims():
    name, tri, cam, views = _case("batch_corner_75x45")
    eg, ed, em, er = mc.constructed_expected(name)
    covered = (em > 0).reshape(len(views), -1).sum(1)
    print("batch (corner): covered %s, rects %s" % (covered.tolist(), er.tolist()))
    for i in (0, 2):
        assert covered[i] > 100 and mc.tile_hits(tri, cam, views[i]).any(1).sum() >= 4
    for i in (1, 3):
        hits = mc.tile_hits(tri, cam, views[i]).any(1)
        assert hits[-1] and not hits[:-1].any() and covered[i] >= 4          # the union box lies in the last (11x5) tile only
        x, y, w, h = er[i]
        assert x >= 64 and y >= 40
    assert np.array_equal(eg[0], eg[2]) and np.array_equal(eg[1], eg[3])


def _limit_claims():
    names = [c[0] for c in CONSTRUCTED]
    assert len(set(names)) == len(names) and not set(names) & {c[0] for c in CASES}
    for name, tri, cam, views in CONSTRUCTED:
        assert cam["width"] <= 150 and cam["height"] <= 117 and len(tri) <= 3000, name
        for view in views:
            u, v, Z = mc.project(tri, cam, view)
            assert Z.min() > 0.01 and max(np.abs(u).max(), np.abs(v).max()) <= 1.0001e8, name


CLAIMS = {"lattice": _lattice_claims, "roof": _roof_claims, "roof_fan": _fan_claims, "stack": _stack_claims, "slivers_huge": _sliver_and_huge_claims, "clamped_out": _clamped_claims,
          "depth_mm": _depth_claims, "batch": _batch_claims, "batch_corner": _corner_claims, "limits": _limit_claims}


@pytest.mark.parametrize("family", list(CLAIMS))
def test_constructed_cases_are_what_they_claim(family):
    """The constructed cases reach what they were built for, shown with meshraster.c alone or a few lines of numpy over the projected boxes."""
    CLAIMS[family]()


@pytest.mark.parametrize("name", ["batch_chip_75x41", "batch_plane_75x41", "batch_corner_75x45"])
def test_header_batch_one_by_one_and_reversed(mr, name):
    _, tri, cam, views = _case(name)
    exp = mc.constructed_expected(name)
    one = [host_render(mr, tri, cam, [v])[1:] for v in views]
    mc.assert_render_equal(tuple(np.concatenate([o[k] for o in one]) for k in range(4)), exp, name + " one by one")
    mc.assert_render_equal(host_render(mr, tri, cam, views[::-1])[1:], tuple(e[::-1] for e in exp), name + " reversed")


def test_vertex_behind_the_camera_invalidates_the_view(mr):
    chip, views = ms.load_mesh("memoryChip2"), ms.view_grid()
    cam = mc.camera(640, 480, mc.F)
    R_bad = mc.view_reaching_behind(chip, views, 0.02)
    with pytest.raises(ValueError):
        ms.render_view(chip, R_bad, 0.02, cam["fx"], cam["fy"], 640, 480)
    vs = [views[3], (R_bad, 0.02), views[4]]
    rc, gray, depth, mask, rects = host_render(mr, chip, cam, vs)
    assert rc == 1
    eg, ed, em, er = mc.expected(chip, cam, vs[:1])
    assert np.array_equal(gray[0], eg[0]) and np.array_equal(depth[0], ed[0]) and np.array_equal(mask[0], em[0]) and np.array_equal(rects[0], er[0])
    assert np.all(gray[1:] == 0x5a) and np.all(depth[1:] == 0x5a) and np.all(mask[1:] == 0x5a) and np.all(rects[1:] == -7)   # nothing written


# ---- argument checks of the C entry points (no device needed up to the point where LMX_ERR_NO_DEVICE is the answer) -----------------------

def _cam(width=640, height=480, f=mc.F, light=mc.LIGHT):
    return _lib.MeshCamera(width, height, f, f, width / 2.0, height / 2.0, (C.c_double * 3)(*light))


def _views(n=2, distance=0.5):
    v = (_lib.MeshView * n)()
    for i in range(n):
        v[i].R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        v[i].distance = distance
    return v


def _render(tri, n_tri, cam, views, n_views, outs=True):
    L = _lib.lib()
    H, W = 480, 640
    g = np.zeros((max(n_views, 1), H, W), np.uint8)
    r = np.zeros((max(n_views, 1), 4), np.int32)
    return L.lmx_mesh_render(0, tri.ctypes.data if tri is not None else None, n_tri, C.byref(cam) if cam is not None else None, views, n_views,
                             g.ctypes.data if outs else None, None, None, r.ctypes.data if outs else None)


def test_mesh_render_argument_checks():
    tri = np.ascontiguousarray(ms.load_mesh("memoryChip2"))
    L = _lib.lib()
    assert _render(None, 10, _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"null" in L.lmx_last_error()
    assert _render(tri, len(tri), None, _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(), None, 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, 0, _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"n_triangles" in L.lmx_last_error()
    assert _render(tri, -3, _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(), _views(), -1) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(width=0), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"camera" in L.lmx_last_error()
    assert _render(tri, len(tri), _cam(height=-4), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(f=float("nan")), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(f=0.0), _views(), 2) == _lib.LMX_ERR_INVALID_ARG
    assert _render(tri, len(tri), _cam(light=(0.0, 0.0, 0.0)), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"light" in L.lmx_last_error()
    v = _views(3)
    v[1].R[4] = float("inf")
    assert _render(tri, len(tri), _cam(), v, 3) == _lib.LMX_ERR_INVALID_ARG and b"view 1" in L.lmx_last_error()
    v = _views(3)
    v[2].distance = float("nan")
    assert _render(tri, len(tri), _cam(), v, 3) == _lib.LMX_ERR_INVALID_ARG and b"view 2" in L.lmx_last_error()
    bad = tri.copy()
    bad[17, 1, 2] = float("nan")
    assert _render(bad, len(bad), _cam(), _views(), 2) == _lib.LMX_ERR_INVALID_ARG and b"triangle 17" in L.lmx_last_error()
    # nothing to do: no device is touched
    assert _render(tri, len(tri), _cam(), _views(), 0) == _lib.LMX_OK
    if not has_gpu():
        assert _render(tri, len(tri), _cam(), _views(), 2) == _lib.LMX_ERR_NO_DEVICE


def test_bank_train_mesh_argument_checks():
    tri = np.ascontiguousarray(ms.load_mesh("memoryChip2"))
    L = _lib.lib()
    nb = NativeBank.from_bank(ms.empty_bank())
    cam, views = _cam(), _views()
    tp = tri.ctypes.data

    def call(bank=nb.h, t=tp, n=len(tri), c=cam, v=views, nv=2, cid=b"obj"):
        return L.lmx_bank_train_mesh(bank, 0, t, n, C.byref(c) if c is not None else None, v, nv, cid, None, None)

    assert call(bank=None) == _lib.LMX_ERR_INVALID_ARG and b"null" in L.lmx_last_error()
    assert call(t=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(c=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(v=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(cid=None) == _lib.LMX_ERR_INVALID_ARG
    assert call(n=0) == _lib.LMX_ERR_INVALID_ARG
    assert call(nv=-2) == _lib.LMX_ERR_INVALID_ARG
    assert call(c=_cam(width=0)) == _lib.LMX_ERR_INVALID_ARG
    assert call(c=_cam(width=8, height=8)) == _lib.LMX_ERR_SHAPE          # lmx_bank_add_template's "source image too small"
    v = _views(2)
    v[0].R[0] = float("nan")
    assert call(v=v) == _lib.LMX_ERR_INVALID_ARG and b"view 0" in L.lmx_last_error()
    assert call(nv=0) == _lib.LMX_OK and L.lmx_bank_num_templates(nb.h, None) == 0
    side = C.POINTER(_lib.RendererParams)()
    assert L.lmx_bank_train_mesh(nb.h, 0, tp, len(tri), C.byref(cam), views, 0, b"obj", None, C.byref(side)) == _lib.LMX_OK
    assert side and side.contents.n_templates == 0 and side.contents.renderer_width == 640 and side.contents.renderer_focal_length_x == mc.F
    L.lmx_renderer_params_free(side)
    if not has_gpu():
        assert call() == _lib.LMX_ERR_NO_DEVICE
    assert L.lmx_bank_num_templates(nb.h, None) == 0
