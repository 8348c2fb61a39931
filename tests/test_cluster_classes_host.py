"""lmx_cluster_matches_classes, the per-class consumer chain on the host (no GPU), on the constructed cases of tests/cluster_class_cases.py:
against the oracle's restatement applied per class (mean similarity) and against the composition of lmx_cluster_matches_scored per class
(caller's values); its refusals; its equality with lmx_cluster_matches for one class; and the function compiled into a stand-alone program
under AddressSanitizer + UBSan.  Everything is compared with array_equal; nothing here has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_class_cases as ccc
from conftest import ROOT
from linemod_pose_estimation_amd import MATCH_DTYPE, _lib, cluster_matches_classes, cluster_matches_scored, merge_raw
from linemod_pose_estimation_amd.detector import CLUSTER_DTYPE, cluster_matches

ALL_CASES = ccc.CASE_NAMES + ("scored",)


def get_case(name):
    return ccc.scored_case() if name == "scored" else ccc.case_by_name(name)


def check(got, want, what):
    c, k, mem = got
    wc, wk, wmem = want
    assert len(c) == len(wc), (what, len(c), len(wc))
    for f in cc.CLUSTER_FIELDS:
        assert np.array_equal(c[f], wc[f]), (what, f)
    assert np.array_equal(k, wk), (what, "cluster_class")
    assert np.array_equal(mem[:len(wmem)], wmem), (what, "members")


def values_for(name, f, n):
    """Per-match values that order the clusters differently from the similarities: few distinct values (ties), some -inf."""
    rng = np.random.default_rng(7000 + 31 * f + len(name))
    v = rng.choice(np.array([-0.25, -0.011, -0.0625, -1.5, -np.inf]), n, p=[0.3, 0.3, 0.2, 0.15, 0.05])
    return np.ascontiguousarray(v, np.float64)


def scored_chain(values):
    def chain(c, s, mc, pos):
        return cluster_matches_scored(mc, values[pos], s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh)
    return chain


@pytest.mark.parametrize("name", ALL_CASES)
def test_case_equals_the_per_class_reference(name):
    case = get_case(name)
    ref = ccc.reference(case)
    for f in range(case.n_frames):
        what = (name, f)
        m = merge_raw(case.records[case.records["frame"] == f])
        for k in cc.FIELDS:
            assert np.array_equal(m[k], ref[f].matches[k]), (what, k)
        values = values_for(name, f, len(m))
        if ref[f].clusters is None:            # a template id outside its class's side-car: refused, and the message names the class
            for v in (None, values):
                with pytest.raises(_lib.LmxError) as e:
                    cluster_matches_classes(m, ccc.as_tuples(case), v)
                assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "class " in str(e.value), what
            continue
        check(cluster_matches_classes(m, ccc.as_tuples(case)), (ref[f].clusters, ref[f].cluster_class, ref[f].members), what)
        check(cluster_matches_classes(m, ccc.as_tuples(case), values), ccc.compose(m, case.classes, scored_chain(values)), what + ("values",))
        sims = m["similarity"].astype(np.float64)
        check(cluster_matches_classes(m, ccc.as_tuples(case), sims), (ref[f].clusters, ref[f].cluster_class, ref[f].members), what + ("similarities as values",))


def test_values_change_the_order_within_a_class():
    case = ccc.case_by_name("params_differ")
    m = ccc.reference(case)[0].matches
    by_sim = cluster_matches_classes(m, ccc.as_tuples(case))
    by_val = cluster_matches_classes(m, ccc.as_tuples(case), values_for("params_differ", 0, len(m)))
    assert not np.array_equal(by_sim[0]["score"], by_val[0]["score"])


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_one_class_equals_cluster_matches(name):
    """With one class and no values the function is lmx_cluster_matches (on the un-classed cases, every match moved to class 0)."""
    case = cc.case_by_name(name)
    ref = cc.reference(case)
    side = [(case.dists, case.rects, case.step, case.rmin, case.rstep, case.thresh)]
    for f in range(case.n_frames):
        if ref[f].clusters is None:
            continue
        m = ref[f].matches.copy()
        m["class_index"] = 0
        c, mem = cluster_matches(m, *side[0])
        got = cluster_matches_classes(m, side)
        check(got, (c, np.zeros(len(c), np.int32), mem[:int(c["member_count"].sum()) if len(c) else 0]), (name, f))
        for k in cc.CLUSTER_FIELDS:
            assert np.array_equal(got[0][k], ref[f].clusters[k]), (name, f, k)


def _call(m, classes, n_classes, cap_c, cap_m, values=None):
    arr, keep = classes
    cl = np.zeros(max(1, cap_c), CLUSTER_DTYPE)
    cls = np.zeros(max(1, cap_c), np.int32)
    mem = np.zeros(max(1, cap_m), np.int32)
    n = C.c_size_t(12345)
    st = _lib.lib().lmx_cluster_matches_classes(m.ctypes.data if len(m) else None, len(m), values.ctypes.data if values is not None else None, arr, n_classes,
                                                cl.ctypes.data, cls.ctypes.data, cap_c, C.byref(n), mem.ctypes.data, cap_m)
    return st, n.value, cl, cls, mem


def test_refusals():
    from linemod_pose_estimation_amd.detector import _class_sidecars
    case = ccc.case_by_name("same_bin")
    m = ccc.reference(case)[0].matches.copy()
    good = ccc.as_tuples(case)
    L = _lib.lib()
    # a negative class index
    bad = m.copy()
    bad["class_index"][2] = -1
    with pytest.raises(_lib.LmxError) as e:
        cluster_matches_classes(bad, good)
    assert e.value.status == _lib.LMX_ERR_INVALID_ARG and "match 2" in str(e.value) and "negative" in str(e.value)
    # every class's parameters are validated as lmx_cluster_matches validates them, also for a class without a match; the class is named
    d, r = case.classes[0].dists, case.classes[0].rects
    for params, word in (((0, 0.5, 0.1, 2), "vote_row_col_step"), ((10, 0.5, 0.1, -1), "cluster_size_thresh"), ((10, 0.5, 0.0, 2), "renderer_radius_step"),
                         ((10, 0.5, float("nan"), 2), "renderer_radius_step"), ((10, float("inf"), 0.1, 2), "renderer_radius_min")):
        for at in (1, 2):
            classes = list(good) + [None]
            classes[at] = (d, r) + params
            with pytest.raises(_lib.LmxError) as e:
                cluster_matches_classes(m, classes)
            assert e.value.status == _lib.LMX_ERR_INVALID_ARG and ("class %d:" % at) in str(e.value) and word in str(e.value), (params, at, str(e.value))
    classes = [good[0], (np.array([0.72, 1e30]), r, 10, 0.5, 0.1, 2)]
    with pytest.raises(_lib.LmxError) as e:
        cluster_matches_classes(m, classes)
    assert "class 1:" in str(e.value) and "template 1" in str(e.value)
    # null arguments
    arr = _class_sidecars(good)
    assert _call(m, arr, 2, 8, 8)[0] == _lib.LMX_OK
    assert L.lmx_cluster_matches_classes(None, len(m), None, arr[0], 2, None, None, 0, C.byref(C.c_size_t()), None, 0) == _lib.LMX_ERR_INVALID_ARG
    assert L.lmx_cluster_matches_classes(m.ctypes.data, len(m), None, None, 2, None, None, 0, C.byref(C.c_size_t()), None, 0) == _lib.LMX_ERR_INVALID_ARG
    assert L.lmx_cluster_matches_classes(m.ctypes.data, len(m), None, arr[0], 2, None, None, 0, None, None, 0) == _lib.LMX_ERR_INVALID_ARG
    assert L.lmx_cluster_matches_classes(m.ctypes.data, len(m), None, arr[0], -1, None, None, 0, C.byref(C.c_size_t()), None, 0) == _lib.LMX_ERR_INVALID_ARG
    cl = np.zeros(8, CLUSTER_DTYPE)
    assert L.lmx_cluster_matches_classes(m.ctypes.data, len(m), None, arr[0], 2, cl.ctypes.data, None, 8, C.byref(C.c_size_t()), None, 0) == _lib.LMX_ERR_INVALID_ARG
    # a side-car with templates and no arrays
    broken = (_lib.ClassSidecar * 2)(arr[0][0], _lib.ClassSidecar(None, None, 2, arr[0][1].params))
    st = _call(m, (broken, None), 2, 8, 8)[0]
    assert st == _lib.LMX_ERR_INVALID_ARG and "class 1:" in L.lmx_last_error().decode()
    # no classes at all, no matches at all
    assert _call(m, arr, 0, 8, 8)[:2] == (_lib.LMX_OK, 0)
    assert _call(m[:0], arr, 2, 0, 0)[:2] == (_lib.LMX_OK, 0)


def test_overflow_reports_the_full_counts():
    from linemod_pose_estimation_amd.detector import _class_sidecars
    case = ccc.case_by_name("class_without_sidecar")
    r = ccc.reference(case)[0]
    m = r.matches
    arr = _class_sidecars(ccc.as_tuples(case))
    n_c, n_m = len(r.clusters), len(r.members)
    assert n_c >= 4 and n_m > n_c
    st, n, cl, cls, mem = _call(m, arr, 3, n_c, n_m)
    assert st == _lib.LMX_OK and n == n_c
    check((cl[:n], cls[:n], mem), (r.clusters, r.cluster_class, r.members), "exact capacity")
    for cap_c, cap_m in ((n_c - 1, n_m), (n_c, n_m - 1), (0, 0), (1, n_m)):
        st, n, cl, cls, mem = _call(m, arr, 3, cap_c, cap_m)
        assert st == _lib.LMX_ERR_OVERFLOW and n == n_c, (cap_c, cap_m)
        msg = _lib.lib().lmx_last_error().decode()
        assert ("%d clusters" % n_c) in msg and ("%d members" % n_m) in msg, msg


def test_class_beyond_n_classes_counts_as_a_class_without_a_sidecar():
    case = ccc.case_by_name("class_without_sidecar")
    r = ccc.reference(case)[0]
    two = ccc.as_tuples(case)[:2]                                # class 2 now lies beyond n_classes, class 1 has no side-car
    c, k, mem = cluster_matches_classes(r.matches, two)
    keep = r.cluster_class == 0
    assert keep.any() and not keep.all()
    assert np.array_equal(k, r.cluster_class[keep]) and np.array_equal(c["score"], r.clusters["score"][keep])
    assert (r.matches["class_index"][mem[:int(c["member_count"].sum())]] == 0).all()


# ---- the function as a stand-alone program under the sanitizers ----------------------------------------------------------------------------
def _bits64(v):
    return int(np.float64(v).view(np.uint64))


def _write_cases(path, items):
    """items: (matches, values or None, classes as ClassCase.classes holds them)."""
    lines = [str(len(items))]
    for m, values, classes in items:
        lines.append("%d %d %d" % (len(m), len(classes), int(values is not None)))
        for e in m:
            lines.append("%d %d %d %d %d" % (e["x"], e["y"], int(np.float32(e["similarity"]).view(np.uint32)), e["template_id"], e["class_index"]))
        if values is not None:
            lines.append(" ".join(str(_bits64(v)) for v in values))
        for s in classes:
            if s is None:
                lines.append("0 1 0 %d 0" % _bits64(1.0))
                continue
            lines.append("%d %d %d %d %d" % (len(s.dists), s.step, _bits64(s.rmin), _bits64(s.rstep), s.thresh))
            lines.append(" ".join(str(_bits64(v)) for v in s.dists))
            lines.append(" ".join(str(int(v)) for v in s.rects.reshape(-1)))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _expected_output(items):
    out = []
    for m, values, classes in items:
        tuples = [None if s is None else (s.dists, s.rects, s.step, s.rmin, s.rstep, s.thresh) for s in classes]
        try:
            c, k, mem = cluster_matches_classes(m, tuples, values)
        except _lib.LmxError as e:
            out += ["%d 0" % e.status] * 2
            continue
        out.append("0 %d" % len(c))
        for i in range(len(c)):
            b, n = int(c["member_begin"][i]), int(c["member_count"][i])
            out.append("%d %d %d %d %d %d %d %d %d %d %d :%s" % ((k[i],) + tuple(c["index"][i]) + tuple(c["rect"][i]) + (int(c["score"][i:i + 1].view(np.uint64)[0]), b, n,
                                                                  "".join(" %d" % v for v in mem[b:b + n]))))
        out.append("%d %d" % (_lib.LMX_ERR_OVERFLOW if len(c) else _lib.LMX_OK, len(c)))
    return out + ["cluster_classes_host ok"]


def test_stand_alone_program_under_address_and_ub_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself: it needs nothing preloaded and takes no notice of what the environment preloads
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    flags = ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__", "-I", hip_include, "-I", os.path.join(ROOT, "include"),
             "-I", os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")]
    exe = str(tmp_path / "cluster_classes_host")
    subprocess.check_call(["g++"] + flags + san + [os.path.join(ROOT, "tests", "cpp", "cluster_classes_host.cpp"), "-o", exe])
    items = []
    for name in ALL_CASES:
        case = get_case(name)
        for f in range(case.n_frames):
            m = ccc.reference(case)[f].matches
            if len(m) > 600:
                m = m[:600]                                      # the text file stays small; the cut list is a case of its own
            items.append((m, None, case.classes))
            items.append((m, values_for(name, f, len(m)), case.classes))
    cases_file = tmp_path / "cases.txt"
    _write_cases(str(cases_file), items)
    res = subprocess.run([exe, str(cases_file)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    got = res.stdout.split("\n")
    assert got[-1] == "" and got[:-1] == _expected_output(items)
