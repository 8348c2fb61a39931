"""The pose chain's decisions without a device: the shared header (csrc/lmx_pose_chain.hpp, built with plain g++ from
tests/cpp/pose_chain_host.cpp) on exported lists written to a file -- the leaders against cluster_leaders, the live range and the frame
lookup, and hostile lists that must give "no job" without an index leaving an array.  Every case runs through the plain build and
through one under AddressSanitizer + UBSan whose arrays hold exactly their capacity; the program itself decides every slot with 64 lanes
and with one and fails when the two differ."""
import subprocess

import numpy as np
import pytest

import pose_chain_cases as pcc
from pose_chain_cases import BROKEN, DEAD, FLAG_BOUNDS, FLAG_CUT, JOB, NO_JOB_BOUNDS, NO_JOB_CLASS

RECTS = [(3, 4, 10, 10), (-7, 9, 5, 5), (0, 0, 0, 0), (1 << 17, -(1 << 17), 8, 8), ((1 << 17) + 1, 0, 8, 8)]     # the last corner is beyond +-2^17


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("pchost")
    if request.param == "sanitized":
        probe = d / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++"] + pcc.SANITIZE + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0 or \
                subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this toolchain has no sanitizer runtime")
    return pcc.build_host(d, sanitize=request.param == "sanitized"), d / "lists.bin"


def sims(n, seed):
    """n distinct similarities below 90"""
    rng = np.random.RandomState(seed)
    return (60.0 + rng.permutation(n) * 0.125).astype(np.float32)


def some_matches(n, seed, template=0, cls=0):
    s = sims(n, seed)
    return pcc.matches_of([(10 + i, 20 - i, s[i], template if i % 3 else 1, cls) for i in range(n)])


def leader_lists():
    """A first frame so that match_begin, cluster_begin and member_begin are not 0, then the frame with the four clusters the leaders are tested on: one member, a tie among five, a tie across the lane stride, the maximum last."""
    m0 = some_matches(7, 1)
    m1 = some_matches(210, 2)
    single = [135]
    five = [130, 131, 132, 133, 134]
    m1["similarity"][[131, 133]] = 95.0                            # positions 1 and 3
    seventy = list(range(209, 139, -1))                            # members in falling match order: position p is match 209 - p
    m1["similarity"][[209 - 64, 209 - 69]] = 97.0                  # positions 64 and 69: lane 0's second member and lane 5's
    big = [int(v) for v in np.random.RandomState(3).permutation(130)]
    m1["similarity"][big[-1]] = 99.0                               # the maximum last
    return pcc.build_lists([(0, m0, [[0, 3], [6]]), (0, m1, [single, five, seventy, big])]), dict(five=3, seventy=4, big=5)


def test_leaders_equal_cluster_leaders(exe):
    L, at = leader_lists()
    live, flags, slots = pcc.run_host(*exe, L, RECTS)
    assert live == 6 and flags == 0
    want = np.concatenate([pcc.frame_leaders(L, 0), pcc.frame_leaders(L, 1)])
    assert [s["leader"] for s in slots] == want.tolist()
    assert all(s["state"] == JOB and s["flags"] == 0 for s in slots)
    assert [s["frame"] for s in slots] == [0, 0, 1, 1, 1, 1]
    mb = int(L.frame_info[1, 0])
    c = L.clusters
    pos = lambda k: L.members[c[k]["member_begin"]:c[k]["member_begin"] + c[k]["member_count"]].tolist().index(slots[k]["leader"] - mb)   # noqa: E731
    assert pos(at["five"]) == 1 and pos(at["seventy"]) == 64 and pos(at["big"]) == 129 and c[2]["member_count"] == 1
    # the job is the leader's match and its template's rect
    for s in slots:
        m = L.matches[s["leader"]]
        assert (s["x"], s["y"], s["template_id"]) == (m["x"], m["y"], m["template_id"]) and (s["rect_x"], s["rect_y"]) == RECTS[m["template_id"]][:2]


def test_signed_zero_and_nan_similarities(exe):
    m = some_matches(6, 4)
    m["similarity"][:4] = (-0.0, 0.0, -1.0, 0.0)
    L = pcc.build_lists([(0, m, [[0, 1, 2, 3]])])
    assert pcc.run_host(*exe, L, RECTS)[2][0]["leader"] == int(pcc.frame_leaders(L, 0)[0]) == 0     # -0 equals 0: the first wins
    m["similarity"][[2, 3]] = np.nan
    L = pcc.build_lists([(0, m, [[0, 1, 2, 3, 4]])])
    assert pcc.run_host(*exe, L, RECTS)[2][0]["leader"] == int(pcc.frame_leaders(L, 0)[0]) == 2     # numpy.argmax: the first NaN


def range_lists():
    frames = [(0, some_matches(9, 5), [[0, 1], [2, 3, 4]]),
              (0, some_matches(4, 6), []),                         # a middle frame without clusters
              (1, some_matches(3, 7), []), (2, some_matches(3, 8), []),
              (4, some_matches(5, 9), [[0, 1], [2]]), (8, some_matches(5, 10), [[4, 3]]),
              (16, some_matches(2, 11), []),
              (0, some_matches(8, 12), [[7], [0, 1, 2], [3, 4, 5, 6]])]
    return pcc.build_lists(frames)


def test_live_range_and_frame_lookup(exe):
    L = range_lists()
    live, flags, slots = pcc.run_host(*exe, L, RECTS)
    assert live == 8 and flags == 0
    assert [s["state"] for s in slots] == [JOB, JOB, DEAD, DEAD, DEAD, JOB, JOB, JOB]
    assert [s["frame"] for s in slots] == [0, 0, -1, -1, -1, 7, 7, 7]
    assert [s["flags"] for s in slots] == [0, 0, FLAG_CUT, FLAG_CUT, FLAG_CUT, 0, 0, 0]        # status 4 and 8: a capacity of the export's cut them
    assert [s["leader"] for s in slots if s["state"] == JOB] == np.concatenate([pcc.frame_leaders(L, 0), pcc.frame_leaders(L, 7)]).tolist()
    assert all(s["leader"] == -1 for s in slots if s["state"] != JOB)
    # header[3] > cap_clusters, the cut inside the last frame: its slots below the cut are dead too, since the export would not have written them
    caps = (len(L.matches), 7, len(L.members))
    live, flags, slots = pcc.run_host(*exe, L, RECTS, caps=caps)
    assert live == 7 and flags == FLAG_CUT
    assert [s["state"] for s in slots] == [JOB, JOB, DEAD, DEAD, DEAD, DEAD, DEAD] and slots[5]["flags"] == slots[6]["flags"] == FLAG_CUT
    # a member range ending beyond cap_members; a match range ending beyond cap_matches
    for caps in ((len(L.matches), 8, len(L.members) - 1), (len(L.matches) - 1, 8, len(L.members))):
        live, flags, slots = pcc.run_host(*exe, L, RECTS, caps=caps)
        assert live == 8 and flags == 0 and [s["state"] for s in slots] == [JOB, JOB, DEAD, DEAD, DEAD, DEAD, DEAD, DEAD], caps
        assert all(s["flags"] == FLAG_CUT for s in slots[5:])
    # header flag 1: nothing is live, whatever the totals say
    H = L.copy()
    H.header[1] = 1
    live, flags, slots = pcc.run_host(*exe, H, RECTS)
    assert live == 8 and flags == FLAG_CUT and all(s["state"] == DEAD and s["leader"] == -1 for s in slots)
    H.header[3] = 0                                                # as the export writes it: the totals are 0
    assert pcc.run_host(*exe, H, RECTS)[:2] == (0, FLAG_CUT)


def test_class_filter_and_class_base(exe):
    m = pcc.matches_of([(1, 2, 70.0, 0, 0), (3, 4, 80.0, 1, 1), (5, 6, 75.0, 1, 0), (7, 8, 60.0, 2, 1)])
    L = pcc.build_lists([(0, m, [[0, 1], [0, 2], [3]])])
    _, _, slots = pcc.run_host(*exe, L, RECTS, class_index=0)
    assert [(s["state"], s["leader"], s["flags"]) for s in slots] == [(NO_JOB_CLASS, 1, 0), (JOB, 2, 0), (NO_JOB_CLASS, 3, 0)]
    _, _, slots = pcc.run_host(*exe, L, RECTS, class_index=-1)
    assert [s["state"] for s in slots] == [JOB, JOB, JOB] and [s["template_id"] for s in slots] == [1, 1, 2]
    _, _, slots = pcc.run_host(*exe, L, RECTS, class_index=0, class_base=[0, 2, 5])          # class_index is ignored, ids are rebased
    assert [(s["state"], s["template_id"]) for s in slots] == [(JOB, 3), (JOB, 1), (NO_JOB_BOUNDS, 0)]           # 2 + 2 = 4: the rect corner beyond 2^17
    assert (slots[0]["rect_x"], slots[0]["rect_y"]) == (1 << 17, -(1 << 17))


def test_hostile_lists_give_no_job(exe):
    def run(change, **kw):
        L = range_lists()
        change(L)
        live, flags, slots = pcc.run_host(*exe, L, RECTS, **kw)
        assert live == 8
        return slots

    def set_cluster(k, field, v):
        def change(L):
            L.clusters[k][field] = v
        return change

    def set_member(i, v):
        def change(L):
            L.members[i] = v
        return change

    def set_match(i, field, v):
        def change(L):
            L.matches[i][field] = v
        return change

    good = run(lambda L: None)
    L0 = range_lists()
    for what, change in (("member_count 0", set_cluster(1, "member_count", 0)), ("member_count negative", set_cluster(1, "member_count", -3)),
                         ("member_count beyond the array", set_cluster(1, "member_count", 1 << 30)), ("member_begin negative", set_cluster(1, "member_begin", -1)),
                         ("member_begin far", set_cluster(1, "member_begin", (1 << 31) - 1)),
                         ("member -1", set_member(3, -1)), ("member == match_count", set_member(4, 9)), ("member far", set_member(2, -(1 << 31)))):
        slots = run(change)
        assert (slots[1]["state"], slots[1]["leader"], slots[1]["flags"]) == (BROKEN, -1, FLAG_BOUNDS), what
        assert slots[:1] + slots[2:] == good[:1] + good[2:], what                     # the others are not touched by it
    lead = good[0]["leader"]
    for what, tid in (("template_id -1", -1), ("template_id == table size", len(RECTS)), ("template_id far", (1 << 31) - 1), ("rect corner", 4)):
        slots = run(set_match(lead, "template_id", tid))
        assert (slots[0]["state"], slots[0]["leader"], slots[0]["flags"]) == (NO_JOB_BOUNDS, lead, FLAG_BOUNDS), what
    # a class outside class_base, and an id outside its class's range (it would be the next class's crop)
    base = [0, 2, 5]
    for what, field, v in (("class 2", "class_index", 2), ("class -1", "class_index", -1), ("id 2 of class 0", "template_id", 2)):
        slots = run(set_match(lead, field, v), class_base=base)
        assert (slots[0]["state"], slots[0]["leader"], slots[0]["flags"]) == (NO_JOB_BOUNDS, lead, FLAG_BOUNDS), what
    assert run(lambda L: None, class_base=base)[0]["state"] == JOB

    # cluster_begin ranges that overlap: frame 7 claims frame 0's second slot and frame 4's two as well
    def overlap(L):
        L.frame_info[7, 2] = 1
    slots = run(overlap)
    assert [(s["state"], s["leader"], s["flags"]) for s in slots[1:4]] == [(BROKEN, -1, FLAG_BOUNDS)] * 3
    assert slots[0] == good[0] and slots[4] == good[4]
    assert [(s["state"], s["flags"]) for s in slots[5:]] == [(DEAD, 0)] * 3            # nobody claims the slots behind them any more

    # negative ranges in frame_info
    for col in range(6):
        def negative(L, col=col):
            L.frame_info[0, col] = -5
        slots = run(negative)
        if col in (2, 3):                                                              # the frame claims nothing
            assert [(s["state"], s["leader"]) for s in slots[:2]] == [(DEAD, -1)] * 2, col
        else:
            assert [(s["state"], s["leader"]) for s in slots[:2]] == [(BROKEN, -1)] * 2, col
    assert len(L0.members) == 18 and L0.frame_info[0, 1] == 9                          # what the indices above rely on
