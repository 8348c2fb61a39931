"""tests/cpp/export_matches_main.cpp, a complete C++ caller of Detector::uploadDevice -> enqueue -> Detector::exportMatches on its own
stream (hipMalloc'ed inputs and outputs, one hipStreamSynchronize) followed by lmx_ctx_collect_clusters on the same enqueue: both printed
results are the same text, and the counts are the oracle's.  The configuration is tests/test_gpu_export_matches.py's, frames A (beyond
2048 raw records) and B."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from linemod_pose_estimation_amd import NativeBank, _lib, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

S, THR, N_T = 160, 45.0, 80


def test_cpp_caller_prints_the_same_result_twice(tmp_path):
    exe = str(tmp_path / "export_matches_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "export_matches_main.cpp"), "-o", exe, "-L", _lib.CSRC, "-llmx", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    bank = synth.make_bank(N_T, seed=91, size_range=(20.0, 36.0))
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(N_T) % 4) + rng.uniform(-0.005, 0.005, N_T)
    rects = np.stack([np.zeros(N_T), np.zeros(N_T), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    frames = [synth.make_scene(bank, S, S, seed=94)[0], synth.make_scene(bank, S, S, seed=93, n_instances=1)[0]]
    NativeBank.from_bank(bank).save_yaml(tmp_path / "obj_templates.yml")
    np.concatenate([dists[:, None], rects.astype(np.float64)], 1).tofile(tmp_path / "sidecar.f64")
    np.stack([np.ascontiguousarray(fr[0]) for fr in frames]).tofile(tmp_path / "bgr.u8")
    np.stack([np.ascontiguousarray(fr[1]) for fr in frames]).tofile(tmp_path / "depth.u16")
    res = subprocess.run([exe, str(tmp_path / "obj_templates.yml"), str(tmp_path / "sidecar.f64"), str(S), str(S), "2", str(tmp_path / "bgr.u8"),
                          str(tmp_path / "depth.u16"), str(THR), "1"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    exported = [ln[len("export "):] for ln in lines if ln.startswith("export ") and " status " not in ln]
    collected = [ln[len("collect "):] for ln in lines if ln.startswith("collect ")]
    assert exported == collected and len(exported) > 300
    od = o.OracleDetector(bank)
    want = []
    for f, fr in enumerate(frames):
        m = od.match([np.ascontiguousarray(s) for s in fr], THR)
        c, _ = o.cluster_matches(m, dists, rects, 10, 0.5, 0.1, 2)
        assert "export frame %d status 0 raw_records %d" % (f, len(od.last_raw())) in lines
        assert "export frame %d matches %d clusters %d" % (f, len(m), len(c)) in lines
        want.append((len(m), len(c), int(c["member_count"].sum())))
    assert lines[0] == "header frames 2 flags 0 matches %d clusters %d members %d" % tuple(sum(w[k] for w in want) for k in range(3))
