"""The arithmetic of lmx_ctx_export_matches_on without a device: linemod_pose_estimation_amd/csrc/lmx_export_pack.hpp (what k_export_plan
and k_export_pack are written with: which frames the large-frame kernel takes, offsets, the fit test per array, status words, header)
compiled with g++ (tests/cpp/export_pack_host.cpp) against a numpy restatement of include/lmx.h's text on constructed count tables, the
same under -fsanitize=address,undefined as a stand-alone program (tests/cpp/export_pack_main.cpp), and the pure builder export_layout.  The device build of the same header is tests/test_gpu_export_matches.py's."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from linemod_pose_estimation_amd import detector as D
from linemod_pose_estimation_amd import export_layout

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
SMALL_MAX, LARGE_MAX = 2048, 16384
CAPACITY = 1 << 17          # of the context's candidate / record lists


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("export_pack")), "libexport_pack.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "export_pack_host.cpp")])
    lib = C.CDLL(so)
    lib.xp_plan.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.xp_plan.restype = C.c_int32
    lib.xp_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                            C.c_void_p, C.c_void_p, C.c_void_p]
    lib.xp_pack.restype = None
    return lib


# ---- a batch as the chain's kernels describe it ---------------------------------------------------------------------------------------------
def small(nm, nc=0, nmem=0):
    """a frame the LDS kernel delivered"""
    return {"row": (nm, nc, nmem, 0), "raw": nm + 3}


def ring():
    """a frame the LDS kernel hands back with status 2"""
    return {"row": (17, 0, 0, 2), "raw": 20}


def big(raw, nm=0, nc=0, nmem=0, status=0):
    """a frame of `raw` > 2048 records; (nm, nc, nmem, status) is what the large-frame kernel says IF it gets the frame"""
    assert raw > SMALL_MAX
    return {"row": (raw, 0, 0, 1), "raw": raw, "large": (nm, nc, nmem, status)}


def tables(frames, max_large):
    """-> counts [F, 4], lcounts [max(1, max_large), 4] as the large-frame kernel would fill them for the frames listed, raw [F], listed frames"""
    counts = np.array([fr["row"] for fr in frames], np.uint32).reshape(-1, 4)
    listed = [f for f, fr in enumerate(frames) if fr["row"][3] == 1 and fr["row"][0] <= LARGE_MAX][:max_large]
    lcounts = np.full((max(1, max_large), 4), 0xdeadbeef, np.uint32)       # rows of parts nobody ran stay garbage
    for i, f in enumerate(listed):
        lcounts[i] = frames[f]["large"]
    return counts, lcounts, np.array([fr["raw"] for fr in frames], np.uint32), listed


# ---- include/lmx.h's text, restated -------------------------------------------------------------------------------------------------------
def restated(frames, max_large, caps, n_cand, n_rec):
    F = len(frames)
    info = np.zeros((F, 8), np.int32)
    header = np.zeros(16, np.uint32)
    header[0], header[5], header[6] = F, n_cand, n_rec
    placed = np.zeros((F, 3), np.int32)
    placed[:, 0] = -1
    if n_cand > CAPACITY or n_rec > CAPACITY:
        header[1] = 1
        info[:, 6] = 16
        return info, header, placed
    listed = [f for f, fr in enumerate(frames) if fr["row"][3] == 1 and fr["row"][0] <= LARGE_MAX][:max_large]
    pos = [0, 0, 0]
    flags = 0
    for f, fr in enumerate(frames):
        res, part = fr["row"], -1
        if f in listed:
            res, part = fr["large"], listed.index(f)
        info[f, 0], info[f, 2], info[f, 4], info[f, 7] = pos[0], pos[1], pos[2], fr["raw"]
        if res[3] != 0:
            info[f, 6] = 2 if res[3] == 2 else 1
            flags |= 2
            continue
        nm, nc, nmem = res[:3]
        fit_m = pos[0] + nm <= caps[0]
        fit_c = pos[1] + nc <= caps[1] and pos[2] + nmem <= caps[2]
        info[f, 1], info[f, 3], info[f, 5] = nm, nc, nmem
        info[f, 6] = (0 if fit_m else 4) | (0 if fit_c else 8)
        flags |= 4 if info[f, 6] else 0
        placed[f] = part, fit_m, fit_c
        pos = [pos[0] + nm, pos[1] + nc, pos[2] + nmem]
    header[1:5] = flags, pos[0], pos[1], pos[2]
    return info, header, placed


def run(shim, frames, max_large, caps, n_cand=5000, n_rec=4000):
    counts, lcounts, raw, listed = tables(frames, max_large)
    F = len(frames)
    lst = np.full(max(1, max_large), -1, np.int32)
    n_listed = shim.xp_plan(counts.ctypes.data, F, max_large, n_cand, n_rec, CAPACITY, lst.ctypes.data)
    overflow = n_cand > CAPACITY or n_rec > CAPACITY
    assert lst[:n_listed].tolist() == ([] if overflow else listed) and (lst[n_listed:] == -1).all()
    info = np.full((F, 8), -7, np.int32)
    header = np.full(16, 0xffffffff, np.uint32)
    placed = np.full((F, 3), -7, np.int32)
    shim.xp_pack(counts.ctypes.data, lcounts.ctypes.data, raw.ctypes.data, F, max_large, n_cand, n_rec, CAPACITY, caps[0], caps[1], caps[2], info.ctypes.data,
                 header.ctypes.data, placed.ctypes.data)
    want = restated(frames, max_large, caps, n_cand, n_rec)
    if overflow:
        want[0][:, 7] = 0
    assert np.array_equal(info, want[0]), (info, want[0])
    assert np.array_equal(header, want[1]), (header, want[1])
    assert np.array_equal(placed, want[2]), (placed, want[2])
    return info, header, placed


BATCH = [small(185, 8, 35), small(0), ring(), small(159, 3, 14), big(2449, 190, 9, 40), small(0), big(16385), big(9000, 0, 0, 0, 2), small(12, 1, 3),
         big(16384, 700, 2, 11)]
TOTALS = {0: (356, 12, 52), 1: (546, 21, 92), 2: (546, 21, 92), 3: (1246, 23, 103)}      # by max_large: frames 4, 7 (status 2), 9 are the ones listed


@pytest.mark.parametrize("max_large", [0, 1, 2, 3, 10])
def test_statuses_offsets_and_totals(shim, max_large):
    info, header, placed = run(shim, BATCH, max_large, (1 << 20,) * 3)
    assert tuple(header[2:5]) == TOTALS[min(max_large, 3)] and header[0] == len(BATCH) and header[1] == 2 and not header[7:].any()
    assert info[:, 6].tolist() == [0, 0, 2, 0, 0 if max_large >= 1 else 1, 0, 1, 2 if max_large >= 2 else 1, 0, 0 if max_large >= 3 else 1]
    assert info[6, 7] == 16385 and not info[6, [1, 3, 5]].any()             # beyond the large-frame kernel: counts 0, the records are reported
    assert placed[:, 0].tolist() == [-1, -1, -1, -1, 0 if max_large >= 1 else -1, -1, -1, -1, -1, 2 if max_large >= 3 else -1]
    # empty frames and frames nobody finished take no room
    assert info[1, 0] == info[2, 0] == info[3, 0] == 185 and info[1, 1] == 0


def test_empty_batch_of_empty_frames(shim):
    info, header, _ = run(shim, [small(0)] * 5, 2, (0, 0, 0), n_cand=0, n_rec=0)
    assert not info[:, :7].any() and header[1] == 0


@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_capacity_equal_to_the_total_and_one_short(shim, which, short):
    frames = [small(185, 8, 35), small(0), small(159, 3, 14)]
    caps = [344, 11, 49]
    caps[which] -= short
    info, header, placed = run(shim, frames, 1, tuple(caps))
    assert tuple(header[2:5]) == (344, 11, 49)
    want_last = 0 if not short else (4 if which == 0 else 8)
    assert info[:, 6].tolist() == [0, 0, want_last] and header[1] == (4 if short else 0)
    assert placed[2].tolist() == [-1, int(not (short and which == 0)), int(not (short and which != 0))]


def test_matches_fit_but_members_do_not_and_later_frames_still_may(shim):
    frames = [small(10, 2, 5), small(20, 3, 30), small(5, 0, 0), small(4, 1, 2)]
    info, header, placed = run(shim, frames, 0, (39, 6, 36))
    # frame 1's members end at 35 <= 36, frame 3's would end at 37: its clusters go unwritten although they fit
    assert info[:, 6].tolist() == [0, 0, 0, 8] and placed[3].tolist() == [-1, 1, 0] and tuple(header[2:5]) == (39, 6, 37) and header[1] == 4
    info, header, placed = run(shim, frames, 0, (30, 6, 34))
    # frame 1's members do not fit; behind it the member offset is past the capacity, so even frame 2's empty cluster range does not
    # (collect_clusters' rule: begin + count <= capacity)
    assert info[:, 6].tolist() == [0, 8, 12, 12] and placed[:, 1].tolist() == [1, 1, 0, 0]
    assert info[3, :6].tolist() == [35, 4, 5, 1, 35, 2]            # begins count what did not fit


def test_all_capacities_zero(shim):
    info, header, placed = run(shim, BATCH, 3, (0, 0, 0))
    assert tuple(header[2:5]) == TOTALS[3] and header[1] == 2 | 4
    assert info[0].tolist() == [0, 185, 0, 8, 0, 35, 4 | 8, 188]
    assert info[1, 6] == 4 | 8 and info[1, 1] == 0        # an empty frame behind a non-empty one: its empty range starts past the capacity
    assert not placed[info[:, 1] > 0, 1].any() and not placed[info[:, 3] > 0, 2].any()


@pytest.mark.parametrize("n_cand,n_rec", [(CAPACITY + 1, 10), (10, CAPACITY + 1), (CAPACITY, CAPACITY)])
def test_list_overflow(shim, n_cand, n_rec):
    info, header, _ = run(shim, BATCH, 3, (1 << 20,) * 3, n_cand=n_cand, n_rec=n_rec)
    if max(n_cand, n_rec) > CAPACITY:
        assert header[1] == 1 and not header[2:5].any() and (info[:, 6] == 16).all() and not info[:, :6].any()
    else:
        assert header[1] == 2 and tuple(header[2:5]) == TOTALS[3]
    assert header[5] == n_cand and header[6] == n_rec


def test_random_tables(shim):
    rng = np.random.default_rng(5)
    for _ in range(300):
        frames = []
        for _ in range(int(rng.integers(1, 17))):
            kind = rng.integers(0, 6)
            if kind <= 2:
                nm = int(rng.integers(0, 300))
                nc = int(rng.integers(0, 9)) if nm else 0
                frames.append(small(nm, nc, int(rng.integers(nc, 4 * nc + 1))))
            elif kind == 3:
                frames.append(ring())
            else:
                raw = int(rng.choice([2049, 5000, LARGE_MAX, LARGE_MAX + 1, 40000]))
                nm = int(rng.integers(0, 3000))
                frames.append(big(raw, nm, int(rng.integers(0, 20)), int(rng.integers(0, 60)), int(rng.choice([0, 0, 0, 2]))))
        max_large = int(rng.integers(0, 5))
        full = run(shim, frames, max_large, (1 << 20,) * 3)[1][2:5]
        caps = tuple(int(rng.choice([0, max(0, int(t) - 1), int(t), int(t) // 2, 1 << 20])) for t in full)
        run(shim, frames, max_large, caps)


def test_tables_under_address_and_ub_sanitizer(tmp_path):
    """tests/cpp/export_pack_main.cpp, built with -fsanitize=address,undefined, walks constructed and random tables from a file as a plain
    child process, every table in a heap block of exactly its size; its printed results are the restatement's."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "export_pack_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC] + san + [os.path.join(ROOT, "tests", "cpp", "export_pack_main.cpp"), "-o", exe])
    rng = np.random.default_rng(11)
    cases = [(BATCH, ml, caps, 5000, 4000) for ml in (0, 1, 3, 10) for caps in ((1 << 20,) * 3, (0, 0, 0), (545, 21, 91))]
    cases.append((BATCH, 3, (1 << 20,) * 3, CAPACITY + 1, 7))
    for _ in range(60):
        frames = [small(int(rng.integers(0, 300)), int(rng.integers(0, 9)), int(rng.integers(0, 30))) if rng.integers(0, 3) else
                  big(int(rng.choice([2049, LARGE_MAX, LARGE_MAX + 1])), int(rng.integers(0, 3000)), int(rng.integers(0, 20)), int(rng.integers(0, 60)),
                      int(rng.choice([0, 0, 2]))) for _ in range(int(rng.integers(1, 17)))]
        cases.append((frames, int(rng.integers(0, 5)), tuple(int(v) for v in rng.integers(0, 2000, 3)), 5000, 4000))
    words, want = [len(cases)], []
    for frames, max_large, caps, n_cand, n_rec in cases:
        counts, lcounts, raw, listed = tables(frames, max_large)
        words += [len(frames), max_large, n_cand, n_rec, CAPACITY] + list(caps) + counts.reshape(-1).tolist() + lcounts.reshape(-1).tolist() + raw.tolist()
        info, header, placed = restated(frames, max_large, caps, n_cand, n_rec)
        overflow = max(n_cand, n_rec) > CAPACITY
        want.append("".join("%d " % f for f in ([] if overflow else listed)) + "| " + " ".join(str(v) for v in info.reshape(-1)) + " | " +
                    " ".join(str(v) for v in header) + " | " + " ".join(str(v) for v in placed.reshape(-1)))
    np.asarray(words, np.uint32).tofile(tmp_path / "cases.u32")
    res = subprocess.run([exe, str(tmp_path / "cases.u32")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "export_pack_main ok %d cases" % len(cases)
    assert lines[:-1] == want


# ---- export_layout ---------------------------------------------------------------------------------------------------------------------------
def test_export_layout_shapes_dtypes_and_sizes():
    lay = export_layout(3, clusters=True, caps=(1000, 40, 77))
    assert list(lay) == ["header", "frame_info", "matches", "clusters", "members"]
    assert lay["header"] == {"shape": (16,), "dtype": "int32", "nbytes": 64, "align": 4, "cap": 16}
    assert lay["frame_info"] == {"shape": (3, 8), "dtype": "int32", "nbytes": 96, "align": 4, "cap": 3}
    assert lay["matches"] == {"shape": (1000, 5), "dtype": "int32", "nbytes": 1000 * D.MATCH_DTYPE.itemsize, "align": 4, "cap": 1000}
    assert lay["clusters"] == {"shape": (40, 48), "dtype": "uint8", "nbytes": 40 * D.CLUSTER_DTYPE.itemsize, "align": 8, "cap": 40}
    assert lay["members"] == {"shape": (77,), "dtype": "int32", "nbytes": 308, "align": 4, "cap": 77}
    assert D.CLUSTER_DTYPE.itemsize == 48 and D.MATCH_DTYPE.itemsize == 20 and len(D.EXPORT_INFO_FIELDS) == D.EXPORT_INFO_WORDS == 8
    assert list(export_layout(1)) == ["header", "frame_info", "matches"] and export_layout(1)["matches"]["cap"] == 1 << 16


def test_export_layout_zero_capacities_keep_an_address():
    lay = export_layout(2, clusters=True, caps=(0, 0, 0))
    for k in ("matches", "clusters", "members"):
        assert lay[k]["cap"] == 0 and lay[k]["shape"][0] == 1 and lay[k]["nbytes"] > 0


@pytest.mark.parametrize("n_frames,caps", [(0, (1, 1, 1)), (1, (-1, 1, 1)), (1, (1, 1 << 31, 1)), (1, (1, 1))])
def test_export_layout_refuses(n_frames, caps):
    with pytest.raises(ValueError):
        export_layout(n_frames, True, caps)


def test_export_desc_mirrors_the_header():
    """The ctypes mirror against the struct in include/lmx.h: the fields in order, and the size a C compiler gives it."""
    from linemod_pose_estimation_amd import _lib
    text = open(os.path.join(ROOT, "include", "lmx.h")).read()
    body = text[text.index("typedef struct lmx_export_desc {"):text.index("} lmx_export_desc;")]
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines()[1:] if ";" in ln]
    assert names == [f[0] for f in _lib.ExportDesc._fields_]
    assert C.sizeof(_lib.ExportDesc) == 16 + 8 * 8
