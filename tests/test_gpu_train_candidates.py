"""The mesh trainer's device path (lmx_bank_train_mesh_opts with LMX_TRAIN_CANDIDATES_DEVICE): k_train_candidates (csrc/lmx_train_cand.hip)
through the hook lmx_debug_train_extract against the CPU build of the header it is written with (tests/test_train_cand_host.py ties that
build to a numpy restatement and to the oracle), on every window of tests/train_select_cases.py and on the shapes where this kernel in
particular can go wrong; then the trainer itself: the device path against the host path -- template ids, templates and features, bank
fingerprint, side-car -- over small meshes, rejections, batch edges, classes, modalities, levels, cut silhouettes, an invalid view, a
fallback view, two runs, the full grid against the committed banks, and a C++ caller."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import train_cand_util as U
import train_select_cases as tc
from conftest import ROOT
from linemod_pose_estimation_amd import NativeBank, _lib, meshsynth as ms

pytestmark = pytest.mark.gpu

F = ms.ENSENSO["fx"]
CASES = tc.all_cases()
WINDOWS = U.windows(CASES)
FAMILIES = sorted({c["family"] for c in CASES})


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return U.build_shim(tmp_path_factory.mktemp("tchost_gpu"))


def _ptr(a):
    return None if a is None else a.ctypes.data


def gpu_extract(w, cap=None):
    """lmx_debug_train_extract -> (status, n, records, header-like words [n, area, counts 8, 0], features or None)"""
    h, wd = w["label"].shape
    cap = h * wd if cap is None else cap
    records = np.zeros((cap + 1, 2), np.uint32)
    n, area, nf, acc = C.c_size_t(0), C.c_uint32(0), C.c_int32(0), C.c_int32(0)
    counts = np.zeros(8, np.uint32)
    feats = np.zeros((64, 3), np.int32)
    st = _lib.lib().lmx_debug_train_extract(0, _ptr(w["label"]), _ptr(w["mag"]), _ptr(w["mask"]), h, wd, w["nf"], w["strong"], w["et"], _ptr(records), cap,
                                            C.byref(n), _ptr(counts), C.byref(area), _ptr(feats), C.byref(nf), C.byref(acc))
    header = np.zeros(U.HEADER_WORDS, np.uint32)
    header[0], header[1], header[2:10] = n.value, area.value, counts
    return st, int(n.value), records, header, (feats[:nf.value].copy() if acc.value else None)


def same_as_cpu(shim, w):
    """-> (candidates, accepted)"""
    n, records, header = U.cpu_list(shim, w)
    st, gn, grecords, gheader, gfeats = gpu_extract(w)
    assert st == _lib.LMX_OK, (w["name"], st, _lib.lib().lmx_last_error())
    assert gn == n and np.array_equal(grecords[:n], records[:n]), (w["name"], gn, n, np.argwhere((grecords[:min(n, gn)] != records[:min(n, gn)]).any(1))[:5])
    assert np.array_equal(gheader[:10], header[:10]), (w["name"], gheader[:10], header[:10])
    feats = U.cpu_select(shim, w, records, header)
    assert (gfeats is None) == (feats is None), w["name"]
    assert feats is None or np.array_equal(gfeats, feats), w["name"]
    return n, feats is not None


@pytest.mark.parametrize("family", FAMILIES)
def test_hook_equals_the_cpu_build_of_the_header(shim, family):
    n = n_acc = n_cands = 0
    for w in WINDOWS:
        if w["family"] == family:
            c, acc = same_as_cpu(shim, w)
            n, n_acc, n_cands = n + 1, n_acc + acc, n_cands + c
    print("%s: %d windows, %d accepted, %d candidates" % (family, n, n_acc, n_cands))
    assert n > 0 and 0 < n_acc < n and n_cands > 0


def test_hook_on_the_shapes_where_the_kernel_can_go_wrong(shim):
    """Widths 1, 2, 3, 5, 63, 65 and heights 1, 2, 7 (dword packing, padding bytes, edge lanes), a uniform label without a mask (every bit
    survives: 1 << 28), the same with 255s and 0s, a 3 x 520 strip (distances up to 519), the largest square window with distances up to
    255, extract_threshold 0, 1 and 2, masks of value 1, 128 and graded; then the window limit and the capacity."""
    names = set()
    for w in U.special_windows():
        same_as_cpu(shim, w)
        names.add(w["name"])
    assert {"uniform_8x8", "sprinkled_8x8", "strip_520x3", "depth_mask_1", "color_mask_128", "depth_1x1_et0", "depth_65x2_et1", "corner_256x256"} <= names
    uniform = [w for w in U.special_windows() if w["name"] == "uniform_8x8"][0]
    st, n, records, _, feats = gpu_extract(uniform)
    assert st == _lib.LMX_OK and n == 64 and (U.decode(records, n)[3] == U.NO_ZERO).all() and feats is not None
    strip = [w for w in U.special_windows() if w["name"] == "strip_520x3"][0]
    st, n, records, _, _ = gpu_extract(strip)
    assert st == _lib.LMX_OK and U.decode(records, n)[3].max() == 519.0
    for shape in ((260, 260), (257, 253)):
        st = gpu_extract(U.window(False, np.full(shape, 4, np.uint8)))[0]
        assert st == _lib.LMX_ERR_SHAPE and b"device path" in _lib.lib().lmx_last_error()
    assert gpu_extract(uniform, cap=63)[0] == _lib.LMX_ERR_OVERFLOW
    assert gpu_extract(uniform, cap=64)[0] == _lib.LMX_OK
    assert gpu_extract(dict(uniform, nf=0))[0] == _lib.LMX_ERR_SHAPE


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------------
def train(tri, views, width, height, f, device, modalities=("ColorGradient", "DepthNormal"), T=(5, 8), cx=None, cy=None, nb=None, class_id="obj"):
    if nb is None:
        b = ms.empty_bank(modalities, T)
        nb = NativeBank.create(b.T, b.modalities)
    meta = nb.train_mesh(tri, views, width, height, f, f, cx, cy, class_id=class_id, device_candidates=device)
    return nb, meta, nb.last_template_ids.copy(), nb.last_side_car, nb.last_train_stats


def same_bank(a, b):
    a, b = a.to_bank(), b.to_bank()
    assert a.T == b.T and [m["type"] for m in a.modalities] == [m["type"] for m in b.modalities]
    ca, cb = sorted(a.classes, key=lambda c: c[0]), sorted(b.classes, key=lambda c: c[0])
    assert [c[0] for c in ca] == [c[0] for c in cb]
    for (cid, ta, fa), (_, tb, fb) in zip(ca, cb):
        assert ta.shape == tb.shape and np.array_equal(ta, tb), (cid, ta.shape, tb.shape)
        assert np.array_equal(fa, fb), cid


def same_training(host, dev, n_views, fallback=0):
    """host, dev: train()'s tuples.  -> the device path's stats"""
    (hb, hmeta, hids, hside, hstats), (db, dmeta, dids, dside, dstats) = host, dev
    assert np.array_equal(dids, hids) and dmeta == hmeta
    same_bank(db, hb)
    fp = _lib.lib().lmx_bank_fingerprint
    assert fp(db.h) == fp(hb.h)
    assert sorted(dside) == sorted(hside)
    for k in hside:
        assert np.array_equal(dside[k], hside[k]), k
    assert (hstats["n_views"], hstats["n_device_views"], hstats["n_fallback_views"], hstats["n_candidates"], hstats["list_bytes"]) == (n_views, 0, 0, 0, 0)
    assert dstats["n_views"] == n_views and dstats["n_accepted"] == hstats["n_accepted"] == len(hmeta)
    assert dstats["n_device_views"] + dstats["n_fallback_views"] == n_views
    assert dstats["n_fallback_views"] == fallback if fallback == 0 else dstats["n_fallback_views"] >= fallback
    assert dstats["list_bytes"] == 64 * dstats["n_device_views"] * len(hb.to_bank().T) * len(hb.to_bank().modalities) + 8 * dstats["n_candidates"]
    return dstats


def both(tri, views, width, height, f, fallback=0, **kw):
    host, dev = train(tri, views, width, height, f, False, **kw), train(tri, views, width, height, f, True, **kw)
    return same_training(host, dev, len(views), fallback), host


SMALL = mc.cases()   # both meshes at 640x480 (61 views each), smaller and off-centre cameras, a silhouette cut by each border, an empty view


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_small_meshes_and_silhouettes_cut_by_each_border(case):
    name, tri, cam, views = case
    stats, host = both(tri, views, cam["width"], cam["height"], cam["fx"], cx=cam["cx"], cy=cam["cy"])
    if name != "chip_cut_outside":
        assert stats["n_candidates"] > 0


@pytest.mark.parametrize("mesh,width,height,div,n_accepted", [("cpu_binary", 224, 160, 3, 56), ("memoryChip2", 160, 120, 4, 61), ("cpu_binary", 320, 240, 2, 201),
                                                            ("cpu_binary", 160, 120, 4, 0)])
def test_rejections_equal_the_host_path(mesh, width, height, div, n_accepted):
    """the configurations of test_rejections_and_order_equal_the_per_view_loop: both accepted and rejected views, resp. none accepted"""
    views = ms.view_grid()[::13]
    stats, host = both(ms.load_mesh(mesh), views, width, height, F / div)
    assert stats["n_accepted"] == n_accepted and len(views) == 204


@pytest.mark.parametrize("n_views", [1, 31, 32, 33, 65])
def test_batch_edges(n_views):
    grid = ms.view_grid()
    views = [grid[i] for i in range(3, 2652, 37)][:n_views]
    assert len(views) == n_views
    stats, _ = both(ms.load_mesh("cpu_binary"), views, 320, 240, F / 2)
    assert stats["n_accepted"] > 0


def test_classes_modalities_and_levels():
    """two classes appended to one bank (and more views to the first); ColorGradient-only and DepthNormal-only banks; three levels at 323x243"""
    chip, cpu, grid = ms.load_mesh("memoryChip2"), ms.load_mesh("cpu_binary"), ms.view_grid()
    views = [grid[i] for i in range(11, 2652, 89)]
    pair = []
    for device in (False, True):
        nb = train(chip, views[:12], 320, 240, F / 2, device, class_id="chip")[0]
        train(cpu, views[:9], 320, 240, F / 2, device, nb=nb, class_id="cpu")
        pair.append(train(chip, views[12:20], 320, 240, F / 2, device, nb=nb, class_id="chip"))
    same_training(pair[0], pair[1], 8)
    assert pair[1][0].class_ids() == ["chip", "cpu"] and list(pair[1][2]) == list(range(12, 20))
    for mods in (("ColorGradient",), ("DepthNormal",)):
        stats, _ = both(chip, views, 320, 240, F / 2, modalities=mods)
        assert stats["n_accepted"] > 0
    stats, _ = both(chip, views, 323, 243, F / 2, T=(5, 8, 10))
    assert stats["n_accepted"] > 0


def test_invalid_view_in_a_later_batch_leaves_the_bank_unchanged():
    chip, grid = ms.load_mesh("memoryChip2"), ms.view_grid()
    views = [grid[i] for i in range(0, 50)]
    bad = views[:40] + [(mc.view_reaching_behind(chip, grid, 0.02), 0.02)] + views[40:]
    texts = []
    for device in (False, True):
        nb = train(chip, views[:5], 320, 240, F / 2, device)[0]
        before = _lib.lib().lmx_bank_fingerprint(nb.h)
        with pytest.raises(_lib.LmxError) as e:
            train(chip, bad, 320, 240, F / 2, device, nb=nb)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "view 40 " in str(e.value)
        assert _lib.lib().lmx_bank_fingerprint(nb.h) == before
        texts.append(str(e.value))
    assert texts[0] == texts[1]


def test_a_close_up_view_falls_back_to_the_host_path():
    """one view whose level-0 window is 322 x 305 pixels (beyond the kernel's window image) among ordinary ones, in the second batch"""
    chip, grid = ms.load_mesh("memoryChip2"), ms.view_grid()
    views = [grid[i] for i in range(5, 2652, 67)]
    views = views[:35] + [(grid[100][0], 0.3)] + views[35:]
    stats, host = both(chip, views, 640, 480, F, fallback=1)
    assert stats["n_fallback_views"] == 1 and stats["n_device_views"] == len(views) - 1


def test_two_device_runs_give_the_same_bytes(tmp_path):
    cpu, views = ms.load_mesh("cpu_binary"), ms.view_grid()[::29]
    a, b = train(cpu, views, 320, 240, F / 2, True), train(cpu, views, 320, 240, F / 2, True)
    a[0].save_yaml(tmp_path / "a.yml")
    b[0].save_yaml(tmp_path / "b.yml")
    assert (tmp_path / "a.yml").read_bytes() == (tmp_path / "b.yml").read_bytes() and len(a[1]) > 0
    assert np.array_equal(a[2], b[2]) and a[4]["n_candidates"] == b[4]["n_candidates"]
    for k in a[3]:
        assert np.array_equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("name", ["memoryChip2", "cpu_binary"])
def test_full_grid_equals_the_committed_bank(name):
    """all 2652 views on the device path: the comparison tests/test_gpu_mesh_train.py makes for the host path, and no view falls back"""
    bank, rects, dists, views_idx = ms.load_bank(name)
    tri, views = ms.load_mesh(name), ms.view_grid()
    nb = NativeBank.create(bank.T, bank.modalities)
    meta = nb.train_mesh(tri, views, device_candidates=True)
    assert [m["view"] for m in meta] == list(views_idx) and len(meta) == 2652
    assert np.array_equal(np.asarray([m["rect"] for m in meta], np.int32), rects)
    assert np.array_equal(np.asarray([m["distance"] for m in meta], np.float32), dists.astype(np.float32))
    assert np.array_equal(nb.last_template_ids, np.arange(2652))
    got = nb.to_bank()
    assert got.T == bank.T
    for (cid, ta, fa), (_, tb, fb) in zip(sorted(got.classes, key=lambda c: c[0]), sorted(bank.classes, key=lambda c: c[0])):
        assert np.array_equal(ta, tb) and np.array_equal(fa, fb), cid
    st = nb.last_train_stats
    print("full grid %s: %s" % (name, st))
    assert st["n_fallback_views"] == 0 and st["n_device_views"] == 2652 and st["n_candidates"] > 0


def test_cpp_caller_with_the_opts_argument_trains_the_same_bank(tmp_path):
    """tests/cpp/mesh_train_opts_main.cpp (Detector::addTemplatesFromMesh with lmx_train_mesh_opts) == Python's host path"""
    exe = str(tmp_path / "mesh_train_opts_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mesh_train_opts_main.cpp"),
                           "-o", exe, "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    cpu = ms.load_mesh("cpu_binary")
    views = ms.view_grid()[::13][:60]
    np.ascontiguousarray(cpu, np.float64).tofile(tmp_path / "tri.f64")
    mc.pack_views(views).tofile(tmp_path / "views.f64")
    res = subprocess.run([exe, str(tmp_path / "tri.f64"), str(tmp_path / "views.f64"), "224", "160", repr(F / 3), str(tmp_path / "out.yml")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    nb, meta, ids, _, _ = train(cpu, views, 224, 160, F / 3, False)
    assert 0 < len(meta) < len(views)
    assert res.stdout.strip().splitlines()[0] == "views %d accepted %d templates %d side_car %d device_views %d fallback_views 0" % (len(views), len(meta), len(meta), len(meta), len(views))
    same_bank(NativeBank.load_yaml(tmp_path / "out.yml"), nb)
