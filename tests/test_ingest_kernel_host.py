"""The ingest kernel of lmx_ctx_upload_device on the CPU: linemod_pose_estimation_amd/csrc/lmx_ingest.hpp (the header k_ingest is written
with: work item, wide and narrow path, the register shifts, the packed blur, BORDER_REFLECT_101 at the row ends) compiled with g++
(tests/cpp/ingest_host.cpp) and run lane by lane over the kernel's grid, pixel for pixel against the oracle's pre_color / pre_depth on
every launch of tests/ingest_cases.py, each with its three frames at three different pitches and bases, twice (two placement lists);
  - the same under -fsanitize=address,undefined as a stand-alone program (tests/cpp/ingest_main.cpp), every source image in a block that
    ends where the image does.
The device build of the same header is tests/test_gpu_device_input.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ingest_cases as ic
from conftest import ROOT
from oracle import oracle as o

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("ingest")), "libingest.so")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "cpp", "ingest_host.cpp")])
    lib = C.CDLL(so)
    lib.ing_run.argtypes = [C.c_int] * 12 + [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ing_frame_bytes.argtypes = [C.c_int] * 6
    lib.ing_frame_bytes.restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def cases():
    return ic.launches(o)


def run(lib, case, layout):
    """-> (frames on the wide path, the frames the launch wrote)"""
    (SW, SH), (cx, cy) = case["size"], case["crop"]
    keep, src, stride = [], [], []
    for (pitch, offset), image in zip(layout, case["frames"]):
        buf, addr = ic.place(image, pitch, offset)
        keep.append(buf)
        src.append(addr)
        stride.append(pitch)
    fb = lib.ing_frame_bytes(case["color"], case["sc"], case["dc"], case["depth_float"], ic.H, ic.W)
    assert fb == case["expected"][0].nbytes
    raw = np.full(fb * len(layout) + 64, ic.FILL, np.uint8)
    at = (-raw.ctypes.data) % 64
    dst = raw[at:at + fb * len(layout)]
    src, stride = np.asarray(src, np.uint64), np.asarray(stride, np.uint64)
    wide = lib.ing_run(case["color"], case["sc"], case["dc"], case["blur"], case["depth_float"], SH, SW, ic.H, ic.W, cx, cy, len(layout),
                       src.ctypes.data, stride.ctypes.data, dst.ctypes.data)
    assert wide >= 0, case["name"]
    assert (raw[:at] == ic.FILL).all() and (raw[at + dst.size:] == ic.FILL).all(), (case["name"], "wrote outside the frames")
    return wide, [dst[f * fb:(f + 1) * fb].view(e.dtype).reshape(e.shape) for f, e in enumerate(case["expected"])]


def test_every_launch_equals_the_oracle_on_both_paths(shim, cases):
    """Placement list A: packed (narrow: 184 and 187 pixels give no 16-byte pitch), packed + one element at an odd base (narrow), 1024 bytes
    at an aligned base (wide).  List B: 1024 bytes at a base 1 to 15 bytes off (narrow), 16 bytes off (wide), packed at an odd base."""
    n_wide = n_narrow = 0
    for ci, case in enumerate(cases):
        for li, layout in enumerate(ic.placements(ic.source_row_bytes(case), ic.element_size(case), ci)):
            wide, got = run(shim, case, layout)
            packed_wide = ic.source_row_bytes(case) % 16 == 0
            assert wide == (1 + packed_wide if li == 0 else 1), (case["name"], li, wide)
            for f, (g, e) in enumerate(zip(got, case["expected"])):
                bad = np.argwhere(g != e)
                assert bad.size == 0, (case["name"], "list", li, "frame", f, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], e[tuple(bad[0])])
            n_wide += wide
            n_narrow += len(layout) - wide
    print("%d launches x 2 placement lists: %d frames on the wide path, %d on the narrow one" % (len(cases), n_wide, n_narrow))
    assert n_wide >= len(cases) and n_narrow >= len(cases)


def test_float_depth_launches_hold_every_special_value(cases):
    """What the float-depth comparisons above stand on: every crop of every frame holds every value of np_restatement's table."""
    import np_restatement as npr
    table = np.unique(npr.pre_depth_special_values()[0].view(np.uint32))
    n = 0
    for case in cases:
        if case["depth_float"]:
            (cx, cy) = case["crop"]
            for z in case["frames"]:
                assert np.array_equal(np.unique(z[cy:cy + ic.H, cx:cx + ic.W].view(np.uint32)), table), case["name"]
                n += 1
    assert n >= 3 * 8


def test_cases_under_address_and_ub_sanitizer(tmp_path, cases):
    """tests/cpp/ingest_main.cpp, built with -fsanitize=address,undefined, runs every launch from a file as a plain child process and
    compares with the expected frames in it; a read past an image's last byte (last granule on the wide path) ends it."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    exe = str(tmp_path / "ingest_main")
    subprocess.check_call(["g++", "-O1"] + FLAGS + san + [os.path.join(ROOT, "tests", "cpp", "ingest_main.cpp"), "-o", exe])
    n = ic.write_cases(tmp_path / "cases.bin", cases)
    res = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "ingest_main ok %d cases" % n and n == 2 * len(cases)
    want = []
    for ci, case in enumerate(cases):
        packed_wide = ic.source_row_bytes(case) % 16 == 0
        want += ["%d wide %d" % (2 * ci, 1 + packed_wide), "%d wide 1" % (2 * ci + 1)]
    assert lines[:-1] == want
