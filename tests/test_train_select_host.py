"""The trainer's host half on the CPU: linemod_pose_estimation_amd/csrc/lmx_train_select.hpp (extractTemplate's ranking, the scattered selection,
the window rule, cropTemplates, and select_pyramid, the one function both trainers call) compiled with g++ into a shim (tests/cpp/
train_select_host.cpp) against the oracle's ColorGradientPyramid / DepthNormalPyramid::extractTemplate and cropTemplates on the label images of
tests/train_select_cases.py: features, their order, template sizes, bounding box, accept / reject, all with array_equal.  The oracle itself is
tied to a brute-force numpy restatement (np_restatement.py: the chessboard distance as an explicit minimum over all zero pixels), because its
chamfer transform and the product's were written alike.  The device half (quantisers, pyramids) is tests/test_gpu_train_sizes.py's."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_restatement as R
import train_select_cases as tc
from conftest import ROOT
from oracle import oracle as o

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
CASES = tc.all_cases()
FAMILIES = sorted({c["family"] for c in CASES})


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tshost") / "libtshost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "cpp", "train_select_host.cpp")])
    lib = C.CDLL(so)
    lib.tsh_extract.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
    lib.tsh_pyramid.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 15 + [C.c_int]
    return lib


@pytest.fixture(scope="module")
def expected():
    """The oracle's answer per case, computed once: None (rejected) or (templates, features, bounding box)."""
    return [o.extract_pyramid(c["mods"], c["labels"], c["mags"], c["masks"]) for c in CASES]


def _ptr(a):
    return None if a is None else a.ctypes.data


def run_pyramid(lib, case, mode, windows=None):
    """tsh_pyramid -> (status, None or (templates, features, bb), error text).  windows: per level (x0, y0, w, h) -- the arrays are cut to
    them and handed over packed, with their offsets, the way the mesh trainer's read-back arrives."""
    mods, L, M = case["mods"], len(case["labels"]), len(case["mods"])
    keep, lab, mag, msk, rows, cols, x0s, y0s = [], [], [], [], [], [], [], []
    for l in range(L):
        h, w = case["labels"][l][0].shape
        x0, y0, ww, wh = (0, 0, w, h) if windows is None else windows[l]
        cut = lambda a: None if a is None else np.ascontiguousarray(a[y0:y0 + wh, x0:x0 + ww])
        rows.append(wh); cols.append(ww); x0s.append(x0); y0s.append(y0)
        for m in range(M):
            a, g = cut(case["labels"][l][m]), cut(case["mags"][l][m])
            keep += [a, g]
            lab.append(_ptr(a)); mag.append(_ptr(g))
        k = None if case["masks"] is None else cut(case["masks"][l])
        keep.append(k)
        msk.append(_ptr(k))
    i32 = lambda v: np.asarray(v, np.int32)
    is_color, nf = i32([m["type"] == "ColorGradient" for m in mods]), i32([m["num_features"] for m in mods])
    strong = np.asarray([m.get("strong_threshold", tc.STRONG) for m in mods], np.float32)
    et = i32([m.get("extract_threshold", 2) for m in mods])
    rows, cols, x0s, y0s = i32(rows), i32(cols), i32(x0s), i32(y0s)
    templates = np.zeros((L * M, 5), np.int32)
    features = np.zeros((max(1, int(np.maximum(nf, 0).sum()) * L), 3), np.int32)
    bb = np.zeros(4, np.int32)
    err = C.create_string_buffer(256)
    st = lib.tsh_pyramid(mode, L, M, _ptr(is_color), _ptr(rows), _ptr(cols), _ptr(x0s), _ptr(y0s), (C.c_void_p * (L * M))(*lab), (C.c_void_p * (L * M))(*mag),
                         (C.c_void_p * L)(*msk), _ptr(nf), _ptr(strong), _ptr(et), _ptr(templates), _ptr(features), _ptr(bb), err, 256)
    out = (templates, features[:int(templates[:, 4].sum())].copy(), tuple(int(v) for v in bb)) if st == 0 else None
    return st, out, err.value.decode()


def same(got, ref, what):
    assert (got is None) == (ref is None), (what, "accepted" if got else "rejected", "oracle: accepted" if ref else "oracle: rejected")
    if ref is not None:
        assert np.array_equal(got[0], ref[0]), (what, got[0], ref[0])
        assert np.array_equal(got[1], ref[1]), (what, np.argwhere((got[1] != ref[1]).any(1))[:5] if got[1].shape == ref[1].shape else (got[1].shape, ref[1].shape))
        assert got[2] == ref[2], (what, got[2], ref[2])


def mask_windows(case):
    """Per level the mask's box grown by 2, clamped: the rule written down a second time (lmx_internal.hpp's mesh_window is the third)."""
    out = []
    for m in case["masks"]:
        h, w = m.shape
        ys, xs = np.nonzero(m)
        if len(ys) == 0:
            out.append((0, 0, min(w, 4), min(h, 4)))
        else:
            x0, y0 = max(0, xs.min() - 2), max(0, ys.min() - 2)
            out.append((int(x0), int(y0), int(min(w, xs.max() + 3) - x0), int(min(h, ys.max() + 3) - y0)))
    return out


def test_oracle_acceptance_shares(expected):
    """The comparison is not about empty cases: in every family the oracle accepts at least a third of the cases and rejects at least one."""
    share = collections.OrderedDict()
    for c, e in zip(CASES, expected):
        a = share.setdefault(c["family"], [0, 0])
        a[0] += e is not None
        a[1] += 1
    for fam, (acc, n) in share.items():
        print("family %-18s accepted %3d of %3d" % (fam, acc, n))
    for fam, (acc, n) in share.items():
        assert 3 * acc >= n and acc < n, (fam, acc, n)


def test_pyramids_rejected_at_level_1_only(shim, expected):
    """odd_dots masks vanish at level 1 (ColorGradient), a 12x12 box leaves DepthNormal 4 pixels there: the oracle accepts level 0 on its own
    and rejects the pyramid; the product adds nothing."""
    n = 0
    for c, ref in zip(CASES, expected):
        if c["family"] == "pyramids" and ("odd_dots" in c["name"] or "level1_only" in c["name"]):
            assert ref is None and ("level1_only" in c["name"] or not c["masks"][1].any())
            assert o.extract_pyramid(c["mods"], c["labels"][:1], c["mags"][:1], c["masks"][:1]) is not None
            assert run_pyramid(shim, c, 1)[0] == 1
            n += 1
    assert n >= 4


@pytest.mark.parametrize("family", FAMILIES)
def test_whole_frame_and_window_rule_equal_the_oracle(shim, expected, family):
    """mode 0: extract_* on the whole frame + crop_templates; mode 1: select_pyramid (the window rule inside); with a mask also select_pyramid on
    the packed windows with their offsets.  All three give what the oracle gives on the whole frame."""
    n = 0
    for c, ref in zip(CASES, expected):
        if c["family"] != family:
            continue
        n += 1
        for mode in (0, 1):
            st, got, _ = run_pyramid(shim, c, mode)
            assert st in (0, 1), (c["name"], mode, st)
            same(got, ref, (c["name"], "mode", mode))
        if c["masks"] is not None:
            st, got, _ = run_pyramid(shim, c, 1, mask_windows(c))
            assert st in (0, 1)
            same(got, ref, (c["name"], "packed windows"))
    assert n > 0


def test_single_images_equal_the_oracles_extract_template(shim):
    """extract_color / extract_depth alone (no crop): the features as selected, in image coordinates."""
    n_acc = 0
    for c in CASES:
        if len(c["labels"]) != 1 or len(c["mods"]) != 1:
            continue
        m, lab, mag = c["mods"][0], c["labels"][0][0], c["mags"][0][0]
        mask = None if c["masks"] is None else c["masks"][0]
        color = m["type"] == "ColorGradient"
        ref = o.extract_color(lab, mag, mask, m["num_features"], m["strong_threshold"]) if color else o.extract_depth(lab, mask, m["num_features"], m["extract_threshold"])
        feats = np.zeros((m["num_features"], 3), np.int32)
        n = shim.tsh_extract(int(color), _ptr(lab), _ptr(mag), _ptr(mask), lab.shape[0], lab.shape[1], m["num_features"], m.get("strong_threshold", 0.0),
                             m.get("extract_threshold", 0), _ptr(feats))
        assert (n < 0) == (ref is None) and n != -2, c["name"]
        if ref is not None:
            assert n == m["num_features"] and np.array_equal(feats, ref), c["name"]
            n_acc += 1
    assert n_acc > 100


def test_zero_features_at_a_level_is_refused_before_any_division(shim):
    """num_features 0, or halved to 0 at a coarser level, is an error status with a message, whole frame or window; never a SIGFPE."""
    for c in tc.family_zero_features():
        for mode in (0, 1):
            st, got, err = run_pyramid(shim, c, mode)
            assert st == 2 and got is None and "num_features" in err, (c["name"], mode, st, err)
    lab, mag = np.full((8, 8), 4, np.uint8), np.full((8, 8), 9000.0, np.float32)
    feats = np.zeros((64, 3), np.int32)
    for color in (0, 1):
        for nf in (0, -1, 64):
            assert shim.tsh_extract(color, _ptr(lab), _ptr(mag), None, 8, 8, nf, 55.0, 0, _ptr(feats)) == -2


def tie_images():
    """<= 40x40: the brute-force distance is O(pixels x zero pixels)"""
    rng = np.random.default_rng(21)
    out = []
    for i in range(48):
        H, W = (int(v) for v in rng.integers(4, 41, 2))
        mask = None if i % 3 == 0 else tc.mask_variants(rng, H, W)[int(rng.integers(1, 21))][1]
        out.append((H, W, mask, int(rng.choice([1, 2, 5, 11, 31]))))
    return rng, out


def test_oracle_equals_the_numpy_restatement():
    """The oracle's erode / chamfer distance / selection / both extractTemplates against np_restatement's brute-force forms."""
    rng, images = tie_images()
    acc = {"color": 0, "depth": 0}
    for i, (H, W, mask, nf) in enumerate(images):
        ang, mag = tc.angles(rng, H, W, 0.9), tc.magnitudes(rng, H, W, 0.8)
        if i % 4 == 0:
            mag = rng.choice(np.asarray([3000.0, 3026.0, 4000.0], np.float32), (H, W))        # ties
        a, b = o.extract_color(ang, mag, mask, nf, tc.STRONG), R.extract_color(ang, mag, mask, nf, tc.STRONG)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), ("color", i)
        acc["color"] += a is not None
        normal = tc.blocks(rng, H, W, int(rng.integers(2, 8)), p255=0.04 * (i % 2))
        if i % 6 == 5:
            normal[:] = 8                                                                        # no zero pixel: the huge distance
        et = i % 4
        a, b = o.extract_depth(normal, mask, nf, et), R.extract_depth(normal, mask, nf, et)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), ("depth", i)
        acc["depth"] += a is not None
    print("oracle == numpy on %d images: accepted %s" % (len(images), acc))
    assert min(acc.values()) * 3 >= len(images) and max(acc.values()) < len(images)


def test_cases_under_address_and_ub_sanitizer(tmp_path, expected):
    """tests/cpp/train_select_main.cpp, built with -fsanitize=address,undefined, runs every case (the zero-feature ones too) from a file as a plain
    child process; its lines are the oracle's answers."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "train_select_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC] + san + [os.path.join(ROOT, "tests", "cpp", "train_select_main.cpp"), "-o", exe])
    zero = tc.family_zero_features()
    tc.write_cases(tmp_path / "cases.bin", CASES + zero)
    res = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "train_select_main ok %d cases" % (len(CASES) + len(zero))
    want = []
    for i, e in enumerate(list(expected) + [2] * len(zero)):
        for mode in (0, 1):
            if e is None or e == 2:
                want.append("%d %d %d" % (i, mode, 1 if e is None else 2))
            else:
                want.append("%d %d 0 bb %d %d %d %d T %s F %s" % ((i, mode) + e[2] + (" ".join(str(v) for v in e[0].reshape(-1)), " ".join(str(v) for v in e[1].reshape(-1)))))
    assert lines[:-1] == want
