"""What lmx_ctx_export_clusters_on adds to the export's arithmetic, without a device: the additions to
linemod_pose_estimation_amd/csrc/lmx_export_pack.hpp compiled with g++ (tests/cpp/export_clusters_pack_host.cpp) against a numpy restatement of
include/lmx.h's text -- diffs and ndiffs follow the matches' fit decision and offsets, cluster_class the clusters' (which the members
decide too) -- and the ctypes mirror of lmx_export_clusters_desc and the pure builder export_clusters_layout."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from linemod_pose_estimation_amd import detector as D
from linemod_pose_estimation_amd import export_clusters_layout, export_layout

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
SMALL_MAX, LARGE_MAX = 2048, 16384
CAPACITY = 1 << 17


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("export_clusters_pack")), "libexport_clusters_pack.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "export_clusters_pack_host.cpp")])
    lib = C.CDLL(so)
    lib.xpc_side.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p]
    lib.xpc_side.restype = None
    lib.xpc_diff_dwords.restype = C.c_uint32
    return lib


def small(nm, nc=0, nmem=0):
    return {"row": (nm, nc, nmem, 0)}


def big(raw, nm=0, nc=0, nmem=0, status=0):
    return {"row": (raw, 0, 0, 1), "large": (nm, nc, nmem, status)}


def tables(frames, max_large):
    counts = np.array([fr["row"] for fr in frames], np.uint32).reshape(-1, 4)
    listed = [f for f, fr in enumerate(frames) if fr["row"][3] == 1 and fr["row"][0] <= LARGE_MAX][:max_large]
    lcounts = np.full((max(1, max_large), 4), 0xdeadbeef, np.uint32)
    for i, f in enumerate(listed):
        lcounts[i] = frames[f]["large"]
    return counts, lcounts, listed


def restated(frames, max_large, caps, has, n_cand, n_rec):
    """include/lmx.h: a frame's range of diffs / ndiffs is written iff the call has the array and the frame's whole match range fits;
    of cluster_class iff its cluster AND member ranges fit; offsets are the matches' / the clusters'; undelivered frames have counts 0."""
    side = np.zeros((len(frames), 8), np.int64)
    if n_cand > CAPACITY or n_rec > CAPACITY:
        side[:, 7] = 16
        return side
    listed = [f for f, fr in enumerate(frames) if fr["row"][3] == 1 and fr["row"][0] <= LARGE_MAX][:max_large]
    pos = [0, 0, 0]
    for f, fr in enumerate(frames):
        res = fr["large"] if f in listed else fr["row"]
        side[f, 0], side[f, 4] = pos[0], pos[1]
        if res[3] != 0:
            side[f, 7] = 2 if res[3] == 2 else 1
            continue
        nm, nc, nmem = res[:3]
        fit_m = pos[0] + nm <= caps[0]
        fit_c = pos[1] + nc <= caps[1] and pos[2] + nmem <= caps[2]
        side[f, 1], side[f, 5] = nm, nc
        side[f, 2], side[f, 3], side[f, 6] = bool(has & 1) and fit_m, bool(has & 2) and fit_m, bool(has & 4) and fit_c
        side[f, 7] = (0 if fit_m else 4) | (0 if fit_c else 8)
        pos = [pos[0] + nm, pos[1] + nc, pos[2] + nmem]
    return side


def run(shim, frames, max_large, caps, has, n_cand=5000, n_rec=4000):
    counts, lcounts, _ = tables(frames, max_large)
    side = np.full((len(frames), 8), -7, np.int64)
    shim.xpc_side(counts.ctypes.data, lcounts.ctypes.data, len(frames), max_large, n_cand, n_rec, CAPACITY, caps[0], caps[1], caps[2], has, side.ctypes.data)
    want = restated(frames, max_large, caps, has, n_cand, n_rec)
    assert np.array_equal(side, want), (side, want)
    return side


BATCH = [small(185, 8, 35), small(0), big(2449, 190, 9, 40), small(159, 3, 14), big(16385), big(9000, 17, 0, 0, 2), small(12, 1, 3)]
TOTAL = (185 + 190 + 159 + 12, 8 + 9 + 3 + 1, 35 + 40 + 14 + 3)       # with max_large >= 1


@pytest.mark.parametrize("has", range(8))
def test_side_arrays_follow_their_parent_with_room_for_everything(shim, has):
    side = run(shim, BATCH, 2, (1 << 20,) * 3, has)
    delivered = side[:, 7] == 0
    assert delivered.tolist() == [True, True, True, True, False, False, True]
    assert (side[delivered, 2] == (has & 1)).all() and (side[delivered, 3] == (has >> 1 & 1)).all() and (side[delivered, 6] == (has >> 2 & 1)).all()
    assert not side[~delivered][:, [1, 2, 3, 5, 6]].any()                  # nothing of a frame nobody finished
    assert side[:, 0].tolist() == [0, 185, 185, 375, 534, 534, 534] and side[:, 4].tolist() == [0, 8, 8, 17, 20, 20, 20]


@pytest.mark.parametrize("which,short", list(itertools.product(range(3), (0, 1))))
def test_capacity_equal_to_the_total_and_one_short(shim, which, short):
    caps = list(TOTAL)
    caps[which] -= short
    side = run(shim, BATCH, 1, tuple(caps), 7)
    last = side[6]
    # one match short: the last frame's diffs and ndiffs go with its matches, cluster_class still arrives; one cluster or one member
    # short: cluster_class goes with the clusters, the diffs still arrive
    assert last[2] == last[3] == int(not (short and which == 0)) and last[6] == int(not (short and which != 0))
    assert last[7] == (0 if not short else (4 if which == 0 else 8))
    assert side[:4, [2, 3, 6]].all() and (last[0], last[1], last[4], last[5]) == (TOTAL[0] - 12, 12, TOTAL[1] - 1, 1)


def test_all_capacities_zero_and_an_empty_frame(shim):
    side = run(shim, [small(0), small(5, 1, 2), small(0)], 0, (0, 0, 0), 7)
    # an empty frame at offset 0 fits a capacity of 0 (begin + 0 <= 0); behind a frame that did not fit it does not
    assert side[:, 2].tolist() == [1, 0, 0] and side[:, 6].tolist() == [1, 0, 0] and side[:, 7].tolist() == [0, 12, 12]


@pytest.mark.parametrize("n_cand,n_rec", [(CAPACITY + 1, 10), (10, CAPACITY + 1), (CAPACITY, CAPACITY)])
def test_list_overflow_writes_nothing(shim, n_cand, n_rec):
    side = run(shim, BATCH, 2, (1 << 20,) * 3, 7, n_cand=n_cand, n_rec=n_rec)
    if max(n_cand, n_rec) > CAPACITY:
        assert (side[:, 7] == 16).all() and not side[:, :7].any()
    else:
        assert side[0, 2] == 1


def test_random_tables(shim):
    rng = np.random.default_rng(23)
    for _ in range(300):
        frames = []
        for _ in range(int(rng.integers(1, 13))):
            if rng.integers(0, 3):
                nm = int(rng.integers(0, 300))
                nc = int(rng.integers(0, 9)) if nm else 0
                frames.append(small(nm, nc, int(rng.integers(nc, 4 * nc + 1))))
            else:
                frames.append(big(int(rng.choice([2049, LARGE_MAX, LARGE_MAX + 1])), int(rng.integers(0, 3000)), int(rng.integers(0, 20)), int(rng.integers(0, 60)),
                                  int(rng.choice([0, 0, 2]))))
        max_large = int(rng.integers(0, 4))
        full = run(shim, frames, max_large, (1 << 20,) * 3, 7)
        tm, tc = int(full[:, 1].sum()), int(full[:, 5].sum())
        caps = (int(rng.choice([0, max(0, tm - 1), tm, tm // 2])), int(rng.choice([0, max(0, tc - 1), tc, 1 << 20])), int(rng.choice([0, 40, 1 << 20])))
        run(shim, frames, max_large, caps, int(rng.integers(0, 8)))


def test_a_diff_record_is_four_dwords(shim):
    assert shim.xpc_diff_dwords() * 4 == D.DEPTH_DIFF_DTYPE.itemsize == D.NORMAL_DIFF_DTYPE.itemsize == 16


# ---- the front end's pure parts -----------------------------------------------------------------------------------------------------------
def test_export_clusters_desc_mirrors_the_header():
    """The ctypes mirror against the struct in include/lmx.h: the fields in order, and the size a C compiler gives it."""
    from linemod_pose_estimation_amd import _lib
    text = open(os.path.join(ROOT, "include", "lmx.h")).read()
    body = text[text.index("typedef struct lmx_export_clusters_desc {"):text.index("} lmx_export_clusters_desc;")]
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines()[1:] if ";" in ln]
    assert names == [f[0] for f in _lib.ExportClustersDesc._fields_]
    assert C.sizeof(_lib.ExportClustersDesc) == 8 * 4 + 14 * 8
    assert C.sizeof(_lib.ExportDesc) == 16 + 8 * 8                        # the older struct is not extended


def test_the_c_compiler_gives_the_struct_the_same_size(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lmx.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(lmx_export_clusters_desc), '
                   'offsetof(lmx_export_clusters_desc, no_value), offsetof(lmx_export_clusters_desc, cap_members)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    from linemod_pose_estimation_amd import _lib
    want = "%d %d %d" % (C.sizeof(_lib.ExportClustersDesc), _lib.ExportClustersDesc.no_value.offset, _lib.ExportClustersDesc.cap_members.offset)
    assert subprocess.check_output([exe], text=True).strip() == want


def test_export_clusters_layout():
    base = export_layout(3, clusters=True, caps=(1000, 40, 77))
    lay = export_clusters_layout(3, score=2, classes=True, caps=(1000, 40, 77))
    assert list(lay) == list(base) + ["diffs", "ndiffs", "cluster_class"] and all(lay[k] == base[k] for k in base)
    assert lay["diffs"] == lay["ndiffs"] == {"shape": (1000, 2), "dtype": "int64", "nbytes": 16000, "align": 8, "cap": 1000}
    assert lay["cluster_class"] == {"shape": (40,), "dtype": "int32", "nbytes": 160, "align": 4, "cap": 40}
    assert list(export_clusters_layout(1)) == list(export_layout(1, clusters=True))
    assert list(export_clusters_layout(1, score=1)) == list(export_layout(1, clusters=True)) + ["diffs"]
    zero = export_clusters_layout(2, 2, True, (0, 0, 0))
    for k in ("diffs", "ndiffs", "cluster_class"):
        assert zero[k]["cap"] == 0 and zero[k]["shape"][0] == 1
    with pytest.raises(ValueError):
        export_clusters_layout(1, score=3)
