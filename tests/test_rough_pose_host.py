"""The rough pose stage without a device: the shared header (csrc/lmx_rough_pose.hpp, built with plain g++ from
tests/cpp/rough_pose_host.cpp) on the lists and view tables of tests/rough_pose_cases.py.  Every case runs through the plain build and
through one under AddressSanitizer + UBSan whose arrays hold exactly their capacity; the records, the member groups and the quaternions
are compared byte for byte with the numpy restatement of the header's comment (rough_pose_cases.np_rough), then with what the case was
built to show.  The program itself decides every slot with 64 lanes and with one, and runs the real std::sort with the reference's
comparator on the groups: it fails when the emulation's winner is not what std::sort leaves first."""
import subprocess

import numpy as np
import pytest

import pose_chain_cases as pcc
import rough_pose_cases as rpc

CASES = rpc.cases()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("rphost")
    if request.param == "sanitized":
        probe = d / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++"] + pcc.SANITIZE + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0 or \
                subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this toolchain has no sanitizer runtime")
    return rpc.build_host(d, sanitize=request.param == "sanitized"), d


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cpu_build_equals_the_restatement(exe, case):
    got = rpc.run_host(*exe, case.L, case.views, case.trace_min, class_index=case.class_index, caps=case.caps)
    want = rpc.np_rough(case.L, case.views, case.trace_min, class_index=case.class_index, caps=case.caps)
    assert got[:4] == want[:4], (got[:4], want[:4])
    for name in rpc.ROUGH_POSE_DTYPE.names:
        assert got[4][name].tobytes() == want[4][name].tobytes(), (name, got[4][name], want[4][name])
    assert got[4].tobytes() == want[4].tobytes() and got[5].tobytes() == want[5].tobytes()
    assert got[6].tobytes() == case.views.q.tobytes()
    case.expect(got[2], got[3], got[4], got[5], case.L)


def test_trace_min_restated():
    from linemod_pose_estimation_amd import _lib, rough_trace_min
    for deg in (0.25, 10.0, 90.0, 179.5):
        assert rough_trace_min(deg) == rpc.trace_min_of(deg)
    for deg in (0.0, 180.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.LmxError) as e:
            rough_trace_min(deg)
        assert e.value.status == _lib.LMX_ERR_INVALID_ARG
