"""tests/cpp/export_clusters_main.cpp, a complete C++ caller of Detector::uploadDevice -> enqueue -> DepthTemplates::uploadSceneDevice ->
Detector::exportClusters (score 2) on its own stream (hipMalloc'ed inputs and outputs, one hipStreamSynchronize) followed by
lmx_ctx_collect_clusters_depth_normal on the same enqueue: both printed results are the same text.  The configuration is
tests/test_gpu_export_matches.py's, frames A (beyond 2048 raw records) and B, with one crop per template."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from linemod_pose_estimation_amd import NativeBank, _lib, synth
from test_gpu_cluster_depth import make_crops

pytestmark = pytest.mark.gpu

S, THR, N_T = 160, 45.0, 80


def test_cpp_caller_prints_the_same_result_twice(tmp_path):
    exe = str(tmp_path / "export_clusters_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "export_clusters_main.cpp"), "-o", exe, "-L", _lib.CSRC, "-llmx", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    bank = synth.make_bank(N_T, seed=91, size_range=(20.0, 36.0))
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(N_T) % 4) + rng.uniform(-0.005, 0.005, N_T)
    rects = np.stack([np.zeros(N_T), np.zeros(N_T), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    frames = [synth.make_scene(bank, S, S, seed=94)[0], synth.make_scene(bank, S, S, seed=93, n_instances=1)[0]]
    crops = make_crops(N_T, 31)
    NativeBank.from_bank(bank).save_yaml(tmp_path / "obj_templates.yml")
    np.concatenate([dists[:, None], rects.astype(np.float64)], 1).tofile(tmp_path / "sidecar.f64")
    np.stack([np.ascontiguousarray(fr[0]) for fr in frames]).tofile(tmp_path / "bgr.u8")
    np.stack([np.ascontiguousarray(fr[1]) for fr in frames]).tofile(tmp_path / "depth.u16")
    np.asarray([(c.shape[1], c.shape[0]) for c in crops], np.int32).tofile(tmp_path / "sizes.i32")
    np.concatenate([c.ravel() for c in crops]).astype(np.uint16).tofile(tmp_path / "crops.u16")
    res = subprocess.run([exe, str(tmp_path / "obj_templates.yml"), str(tmp_path / "sidecar.f64"), str(S), str(S), "2", str(tmp_path / "bgr.u8"),
                          str(tmp_path / "depth.u16"), str(THR), "1", str(tmp_path / "sizes.i32"), str(tmp_path / "crops.u16"), "520"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    exported = [ln[len("export "):] for ln in lines if ln.startswith("export ") and " status " not in ln]
    collected = [ln[len("collect "):] for ln in lines if ln.startswith("collect ")]
    assert exported == collected and len(exported) > 300
    status = [ln for ln in lines if " status " in ln]
    assert len(status) == 2 and all(" status 0 " in ln for ln in status) and int(status[0].split()[-1]) > 2048 > int(status[1].split()[-1]) > 0
    assert any(" depth " in ln and int(ln.split(" depth ")[1].split()[1]) > 0 for ln in exported)        # some match had something to compare
    assert lines[0].startswith("header frames 2 flags 0 matches ")
