"""Inputs that send every size-capped loop of the pose-side kernels into a later trip, and what the CPU builds of the shared headers give
for them: shared by tests/test_second_trip_cases_host.py (which proves on the CPU that each shape crosses its cap and that the expected
bytes depend on what only a later trip reads) and tests/test_gpu_second_trips.py (the kernels against those bytes).

The caps are read from the compiled shims (sf_host_launch_caps, nv_host_launch_caps, dv_host_launch_caps): no number of
csrc/lmx_scene_filter.hpp, lmx_normal_verify.hpp or lmx_depth_verify.hpp is repeated here.  What is repeated is the workgroup of 256 lanes
every one of these kernels is launched with.

  loop                                               cap                                      first input of a later trip
  k_scene_filter_score: tiles of a frame             score_grid workgroups                    tile score_grid
  k_scene_filter_apply: pixels of a frame            apply_grid * 256                         flat pixel apply_grid * 256
  k_normal_map_frames: pixels of a frame             frame_map_grid * 256                     flat pixel frame_map_grid * 256
  k_normal_map_crops: elements h * pitch of a crop   crop_map_grid * 256                      element crop_map_grid * 256
  k_depth_crop: vectors h * pitch / 8 of a crop      crop_copy_grid * 256                     vector crop_copy_grid * 256
  diff_walk, crop_pixels: vectors of a crop row      walk_lanes                               column walk_lanes * 8"""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np

import mesh_cases as mc
import normal_verify_cases as nvc
import pose_refine_cases as prc
import pose_refine_plane_cases as ppc
import pose_refine_staged_cases as psc
import pose_verify_cases as pvc
import scene_filter_cases as sfc

WORKGROUP = 256
DV_SRC = os.path.join(prc.ROOT, "tests", "cpp", "depth_verify_host.cpp")


class Hosts:
    """The CPU builds of the headers, compiled into `directory` (the pose headers when first asked for), and the caps of the launches."""

    def __init__(self, directory):
        self.dir = str(directory)
        vp = C.c_void_p
        self.sf = sfc.build_host(self.dir)
        self.nv = nvc.build_host_lib(self.dir)
        so = os.path.join(self.dir, "libdvhost.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", prc.CSRC, "-fPIC", "-shared", "-o", so, DV_SRC])
        self.dv = C.CDLL(so)
        self.dv.dv_host_diff.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]
        self.dv.dv_host_diff.restype = None
        sf, nv, dv = (np.zeros(4, np.int32) for _ in range(3))
        for lib, name, out in ((self.sf, "sf_host_launch_caps", sf), (self.nv, "nv_host_launch_caps", nv), (self.dv, "dv_host_launch_caps", dv)):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = [vp], None
            fn(out.ctypes.data)
        self.caps = SimpleNamespace(tile_w=int(sf[0]), tile_h=int(sf[1]), score_grid=int(sf[2]), apply_grid=int(sf[3]), frame_map_grid=int(nv[0]),
                                    crop_map_grid=int(nv[1]), crop_copy_grid=int(dv[0]), walk_lanes=int(dv[1]), vector=int(dv[2]))
        assert min(vars(self.caps).values()) > 0, self.caps
        self._pose = {}
        self._table = None

    def pose(self, name):
        """"pr", "prs", "prp", "pv": the CPU build of that pose header."""
        if name not in self._pose:
            build = {"pr": prc.build_host, "prs": psc.build_host, "prp": ppc.build_host, "pv": pvc.build_host}[name]
            self._pose[name] = build(self.dir)
        return self._pose[name]

    def angle_table(self):
        if self._table is None:
            self._table = np.zeros(16385, np.uint32)
            self.nv.nv_host_table(self._table.ctypes.data)
        return self._table


# ---- the scene filter ------------------------------------------------------------------------------------------------------------------------------

def tiles_of(W, H, caps):
    return ((W + caps.tile_w - 1) // caps.tile_w, (H + caps.tile_h - 1) // caps.tile_h)


def tile_index(W, H, caps):
    """int64 [H, W]: the tile of each pixel, numbered as k_scene_filter_score numbers them."""
    Y, X = np.mgrid[0:H, 0:W]
    return (Y // caps.tile_h) * tiles_of(W, H, caps)[0] + X // caps.tile_w


def blank_later_tiles(frame, caps):
    out = frame.copy()
    out[tile_index(frame.shape[1], frame.shape[0], caps) >= caps.score_grid] = 0
    return out


def blank_from_pixel(frame, first):
    out = frame.copy()
    out.reshape(-1)[first:] = 0
    return out


class FilterCase:
    """frames of one size for one upload; `tiles` / `pixels`: whether the score loop / the apply loop is meant to take a later trip."""

    def __init__(self, name, frames, r, k, mul, tiles, pixels):
        self.name, self.frames, self.r, self.k, self.mul, self.tiles, self.pixels = name, frames, r, k, mul, tiles, pixels
        self.cam = sfc.scene_camera(frames[0])
        self._want = None

    @property
    def shape(self):
        return self.frames[0].shape[::-1]

    def want(self, hosts):
        """[(filtered map, record array [1])] per frame by the header, computed once."""
        if self._want is None:
            self._want = [filter_by_header(hosts, f, self.cam, self.r, self.k, self.mul) for f in self.frames]
        return self._want


def filter_by_header(hosts, frame, cam, r, k, mul):
    rc, out, rec = sfc.host_filter(hosts.sf, frame, cam, r, k, mul)
    assert rc == 0
    return out, rec


def filter_cases(caps):
    tw, th = caps.tile_w, caps.tile_h
    out = []
    # two tile columns, the right one cut at a quarter of a tile; rows of tiles until both the tile cap and the pixel cap are crossed
    W = tw + tw // 4
    rows = max(caps.score_grid // 2 + 1, (caps.apply_grid * WORKGROUP) // (W * th) + 1)
    far = sfc.noisy(W, th * rows, 8, holes=0.2, spikes=300)
    far[far != 0] += 300
    out.append(FilterCase("two_frames", [sfc.noisy(W, th * rows, 7, holes=0.02, spikes=400), far], 3, 15, 1.0, True, True))
    # the last row of tiles cut at half a tile, just over the tile cap, the largest halo
    out.append(FilterCase("cut_rows_r7", [sfc.noisy(W, th * (caps.score_grid // 2) + th // 2, 9, holes=0.02, spikes=250)], 7, 100, 1.0, True, False))
    # one column of whole tiles, one more than the cap: the last workgroup's worth of pixels is the last tile, not one row along the border
    ty = caps.score_grid + 1
    one_over = sfc.noisy(tw, th * ty, 10, holes=0.02, spikes=400)
    for mul in (0.0, 16.0):
        out.append(FilterCase("one_tile_over_mul_%g" % mul, [one_over], 3, 15, mul, True, tw * th * ty > caps.apply_grid * WORKGROUP))
    return out


def reduced_filter_frames(caps):
    """-> [(frame, r, k)]: one cut frame small enough for scene_filter_cases.np_filter, per radius of the cases."""
    W, H = caps.tile_w + caps.tile_w // 4, 2 * caps.tile_h + caps.tile_h // 2
    return [(sfc.noisy(W, H, 21, holes=0.02, spikes=8), 3, 15), (sfc.noisy(W, H, 22, holes=0.02, spikes=8), 7, 100)]


# ---- the normal maps -------------------------------------------------------------------------------------------------------------------------------

def normal_frame_shape(caps):
    """The first odd width from 1025 on at which some height gives frame_map_grid + 1 workgroups' worth of pixels, ragged at the end."""
    cap = caps.frame_map_grid * WORKGROUP
    for W in range(1025, 4 * 1025, 2):
        H = cap // W + 1
        if W * H <= cap + WORKGROUP:
            return W, H
    raise AssertionError("no frame of %d + 1 workgroups" % caps.frame_map_grid)


def sawtooth_image(w, h, rng):
    """Ramps of 3 mm a column and -2 mm a row that start again every 200 columns and 150 rows (taps across a step do not count), noise, a
    tenth holes, a band beyond the distance threshold; the slopes stay below the tap limit everywhere else, the last row included."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = 900 + 3 * (xx % 200) - 2 * (yy % 150) + rng.integers(-12, 13, (h, w))
    d[h // 3: h // 3 + 3, :] = nvc.DIST_T + 5
    d = d.astype(np.uint16)
    d[rng.random((h, w)) < 0.1] = 0
    return d


def normal_frames(caps):
    """Two frames of normal_frame_shape: sawtooth_image, and the same turned by half a turn."""
    W, H = normal_frame_shape(caps)
    a = sawtooth_image(W, H, np.random.default_rng(31))
    return [a, np.ascontiguousarray(a[::-1, ::-1])]


def normal_crops(caps):
    """-> (crops, index of the first crop meant to cross the cap).  A few small ones; 129 and 520 wide at the larger of 65 / 17 rows and
    the first height with a whole row above the cap; 129 wide above twice the cap."""
    cap = caps.crop_map_grid * WORKGROUP
    rng = np.random.default_rng(32)
    small = [(9, 12), (65, 23), (7, 3)]
    pitch = lambda w: (w + caps.vector - 1) // caps.vector * caps.vector
    big = [(129, max(65, cap // pitch(129) + 2)), (520, max(17, cap // pitch(520) + 2)), (129, 2 * cap // pitch(129) + 2)]
    return [nvc.scene_image(w, h, rng) for w, h in small + big], len(small)


def blank_crop_from_element(crop, first, caps):
    """The crop without the pixels whose element index in its [h][pitch] layout is >= first."""
    h, w = crop.shape
    pitch = (w + caps.vector - 1) // caps.vector * caps.vector
    Y, X = np.mgrid[0:h, 0:w]
    out = crop.copy()
    out[Y * pitch + X >= first] = 0
    return out


# ---- the crop copy of from_mesh --------------------------------------------------------------------------------------------------------------------

MESH_T0 = 100.0    # the mesh lies this far down its own z axis, so that a small turn of a view swings it out of the frame (mesh_cases.view_at)


def mesh_crop_case(caps):
    """A quad whose silhouette box has 33 vectors a row (three columns short of them: the padding rule) and the first height at which
    h * 33 passes the cap, seen as a whole, from four times as far, and swung out of the frame -> (triangles, camera, views, (w, h))."""
    vpr = 2 * caps.crop_copy_grid + 1
    w, h = caps.vector * vpr - 3, caps.crop_copy_grid * WORKGROUP // vpr + 1
    cam = mc.dyadic_camera(w + 27, h + 11)
    x0, y0 = 12.0, 5.0
    corners = [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)]
    Z = [1.0, 1.5, 2.0, 1.25]
    v = mc.place(corners, Z, cam, MESH_T0)
    tri = np.ascontiguousarray(np.stack([v[[0, 1, 2]], v[[0, 2, 3]]]))
    views = [(np.eye(3), 3.0 + MESH_T0), (np.eye(3), MESH_T0), (mc.rot_y(0.1), MESH_T0)]
    return tri, cam, views, (w, h)


# ---- crops wider than one trip of a wave's lanes along a row -----------------------------------------------------------------------------------------

WIDE_ROWS = 14


def wide_surface(X, Y):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return 900.0 + 0.05 * X + 0.8 * Y + 6.0 * np.sin(X / 37.0) + 4.0 * np.cos(Y / 2.1 + X / 90.0)


def wide_case(caps):
    """Crops of one vector more than a trip (one lane takes a second) and of one pixel more than two trips (three trips, a ragged last
    vector), of a gently curved surface moved by less than a pixel and 3 mm, in a scene of that surface: inside, over the right border, over
    the left.  Six rows give the crops' rows 0 and 5 their normals (the taps lie 5 apart)."""
    trip = caps.walk_lanes * caps.vector
    sizes = [(trip + caps.vector, 6), (2 * trip + 1, 6), (2 * trip + 1, 3)]
    W, H = 2 * trip + 1 + 75, WIDE_ROWS
    rng = np.random.RandomState(41)
    Y, X = np.mgrid[0:H, 0:W]
    scene = np.rint(wide_surface(X, Y)).astype(np.uint16)
    scene[rng.rand(H, W) < 0.1] = 0
    cam = (1000.0, 1000.0, W / 2.0, H / 2.0)
    crops, rects, rows = [], [], []
    for k, (w, h) in enumerate(sizes):
        at = (40, 4)
        j, i = np.meshgrid(np.arange(w), np.arange(h))
        c = np.rint(wide_surface(at[0] + j + 0.7, at[1] + i - 0.4) + 3.0).astype(np.uint16)
        c[rng.rand(h, w) < 0.1] = 0
        crops.append(c)
        rects.append(at + (w, h))
        rows += [(at[0], at[1], k), (W - w // 2, at[1], k), (-(w // 2), at[1], k)]
    P = prc.make_params(cam, cam, max_dist_mm=12.0, max_iterations=6, min_pairs=3, search_radius=1)
    return SimpleNamespace(trip=trip, sizes=sizes, scene=scene, cam=cam, crops=crops, rects=np.asarray(rects, np.int32), rows=np.asarray(rows, np.int64), P=P,
                           stages=psc.parse_schedule("4:3:12:2,1:3:12:1"), shifts=[8, 4], PV=pvc.make_params(cam, cam), chain_crop=1)


def blank_from_column(crop, first):
    out = crop.copy()
    out[:, first:] = 0
    return out


def wide_reference(hosts, case, crops, dtypes):
    """What the headers give for every row of the case with `crops` in place of the case's own -> SimpleNamespace of
    diff int64 [n, 3], ndiff int64 [n, 5], refine / staged / plane: lists of (record [1], sums[, plane sums]), verify: list of records [1] of the
    unstaged refine's pose.  dtypes: (POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE)."""
    scene = case.scene
    H, W = scene.shape
    fx, fy = case.cam[0], case.cam[1]
    scene_n = nvc.host_map(hosts.nv, scene, fx, fy)
    scene_p = nvc.packed(scene_n)
    table = hosts.angle_table()
    out = SimpleNamespace(diff=[], ndiff=[], refine=[], staged=[], plane=[], verify=[], scene_normals=scene_n)
    crop_p = [nvc.packed(nvc.host_map(hosts.nv, c, fx, fy)) for c in crops]
    for x, y, k in case.rows:
        c = np.ascontiguousarray(crops[k])
        h, w = c.shape
        rect = case.rects[k, :2]
        d, n = np.zeros(3, np.int64), np.zeros(5, np.int64)
        hosts.dv.dv_host_diff(c.ctypes.data, w, h, w, scene.ctypes.data, W, H, W, int(x), int(y), 0, d.ctypes.data)
        hosts.nv.nv_host_diff(c.ctypes.data, crop_p[k].ctypes.data, w, h, w, scene.ctypes.data, scene_p.ctypes.data, W, H, W, int(x), int(y), table.ctypes.data, n.ctypes.data)
        out.diff.append(d)
        out.ndiff.append(n)
        out.refine.append(prc.host_refine(hosts.pose("pr"), case.P, c, rect, scene, x, y, dtypes[0]))
        out.staged.append(psc.host_refine_staged(hosts.pose("prs"), case.P, case.stages, c, rect, scene, x, y, dtypes[0]))
        out.plane.append(ppc.host_refine_plane(hosts.pose("prp"), case.P, case.stages, case.shifts, c, rect, scene, scene_n, x, y, dtypes[0]))
        pose = out.refine[-1][0]
        if pose["status"][0] == prc.NONE:
            out.verify.append(np.zeros(1, dtypes[1]))
        else:
            out.verify.append(pvc.host_verify(hosts.pose("pv"), case.PV, c, rect, scene, pose["R"][0].reshape(9), pose["t_mm"][0], dtypes[1]))
    out.diff, out.ndiff = np.asarray(out.diff), np.asarray(out.ndiff)
    return out
