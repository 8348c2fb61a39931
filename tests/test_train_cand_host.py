"""The candidate lists of the mesh trainer's device path on the CPU: linemod_pose_estimation_amd/csrc/lmx_train_cand.hpp (the header the kernel
k_train_candidates is written with: candidate rule, the chessboard distance by AND steps on packed bit-planes, record and header format)
compiled with g++ (tests/cpp/train_cand_host.cpp), on every level and modality of every case of tests/train_select_cases.py:
  - the list -- positions in raster order, labels, scores, label counts, area -- equals a numpy restatement of the definitions that uses
    np_restatement's brute-force chessboard distance;
  - what rank_select_color / rank_select_depth (lmx_train_select.hpp) pick from the list equals the oracle's extractTemplate, accepted or
    rejected alike;
  - the same under -fsanitize=address,undefined as a stand-alone program (tests/cpp/train_cand_main.cpp).
The device build of the same header is tests/test_gpu_train_candidates.py's."""
import collections
import os
import subprocess

import numpy as np
import pytest

import train_cand_util as U
import train_select_cases as tc
from conftest import ROOT
from oracle import oracle as o

CASES = tc.all_cases()
WINDOWS = U.windows(CASES)
FAMILIES = sorted({c["family"] for c in CASES})


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return U.build_shim(tmp_path_factory.mktemp("tchost"))


@pytest.fixture(scope="module")
def restated():
    return [U.restate(w) for w in WINDOWS]


@pytest.fixture(scope="module")
def expected():
    """The oracle's extractTemplate per window: None (rejected) or the features."""
    return [o.extract_color(w["label"], w["mag"], w["mask"], w["nf"], w["strong"]) if w["color"] else o.extract_depth(w["label"], w["mask"], w["nf"], w["et"])
            for w in WINDOWS]


def test_oracle_acceptance_shares(expected):
    """In every family the oracle accepts (every level of) at least a third of the cases and rejects at least one: an "all rejected" run
    cannot pass the comparisons below."""
    ok = collections.OrderedDict()
    for w, e in zip(WINDOWS, expected):
        ok[w["case"]] = ok.get(w["case"], True) and e is not None
    share = collections.OrderedDict()
    for ci, acc in ok.items():
        a = share.setdefault(CASES[ci]["family"], [0, 0])
        a[0] += acc
        a[1] += 1
    for fam, (acc, n) in share.items():
        print("family %-18s accepted %3d of %3d" % (fam, acc, n))
        assert 3 * acc >= n and acc < n, (fam, acc, n)
    assert sorted(share) == FAMILIES


@pytest.mark.parametrize("family", FAMILIES)
def test_lists_equal_the_restatement_and_selection_equals_the_oracle(shim, restated, expected, family):
    n = n_acc = n_huge = n_cands = 0
    for w, ref, exp in zip(WINDOWS, restated, expected):
        if w["family"] != family:
            continue
        got = U.cpu_list(shim, w)
        U.same_list(got, ref, w["name"])
        feats = U.cpu_select(shim, w, got[1], got[2])
        assert (feats is None) == (exp is None), (w["name"], "accepted" if feats is not None else "rejected")
        if exp is not None:
            assert np.array_equal(feats, exp), w["name"]
            n_acc += 1
        n += 1
        n_cands += got[0]
        n_huge += int((ref[3] == U.NO_ZERO).sum())
    print("%s: %d windows, %d accepted, %d candidates, %d of them without a zero pixel in their plane" % (family, n, n_acc, n_cands, n_huge))
    assert n > 0 and 0 < n_acc < n and n_cands > 0


def test_special_shapes(shim):
    """The shapes tests/test_gpu_train_candidates.py runs on the device, on the CPU build: narrow and low windows (dword packing, padding
    bytes), planes without a zero pixel (1 << 28), a strip with distances above 255, thresholds 0 and 1, mask values 1 and 128, a window
    beyond the device path's size."""
    n_huge = 0
    for w in U.special_windows():
        ref = U.restate(w)
        U.same_list(U.cpu_list(shim, w), ref, w["name"])
        n_huge += int((ref[3] == U.NO_ZERO).sum())
    assert n_huge >= 64
    strip = [w for w in U.special_windows() if w["name"].startswith("strip")][0]
    assert U.restate(strip)[3].max() == 519.0
    assert U.cpu_list(shim, U.window(False, np.full((260, 260), 4, np.uint8)))[0] == -1     # 65 dwords x 260 rows > 16384
    assert U.cpu_list(shim, U.window(False, np.full((257, 253), 4, np.uint8)))[0] == -1     # 64 dwords x 257 rows: one row too many


def test_cases_under_address_and_ub_sanitizer(tmp_path, restated, expected):
    """tests/cpp/train_cand_main.cpp, built with -fsanitize=address,undefined, runs every window from a file as a plain child process; its
    lines carry the restatement's counts and the oracle's features."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "train_cand_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", U.CSRC] + san + [os.path.join(ROOT, "tests", "cpp", "train_cand_main.cpp"), "-o", exe])
    tc.write_cases(tmp_path / "cases.bin", CASES)
    res = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "train_cand_main ok %d cases" % len(CASES)
    want = []
    for w, ref, exp in zip(WINDOWS, restated, expected):
        level, mod = (int(v[1:]) for v in w["name"].split("/")[-2:])
        head = "%d %d %d %d %d" % (w["case"], level, mod, len(ref[0]), ref[5])
        want.append(head + (" -1" if exp is None else " %d F %s" % (len(exp), " ".join(str(v) for v in exp.reshape(-1)))))
    assert lines[:-1] == want
