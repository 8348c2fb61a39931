"""One-frame lmx_match calls with PAUSES between them (-m gpu).  The call hands the rest of its kernel chain to a helper thread that spins for
300 us behind a job and then sleeps (csrc/lmx_launch_helper.hpp); every other one-frame test calls back to back and so only ever meets the
helper awake.  Here the pauses are drawn around the spin limit, so the calls fall on both sides of -- and into -- the helper's spin-to-sleep
transition, where a wake-up could be lost and the call would never return (tests/test_launch_helper_host.py stresses the class alone, on
the CPU).  The loop runs in a child process with a timeout (tests/one_frame_pauses_child.py): a hung hand-off is a failed test.

The helper's counters (lmx_debug_launch_helper_counters) say which hand-offs the loops really had -- and that the helper path was taken at
all: LMX_NO_LAUNCH_THREAD, profiling or a context without streamed stores would leave them at zero."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from linemod_pose_estimation_amd import Detector, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

CALLS = 4000
# The child's own busy-wait.  What the helper sees is longer: its job ends about half-way through a call, and the rest of the call and Python's
# time around it come before the pause.  Measured with the child's `hist` argument over pauses of 0 .. 700 us: the calls behind a pause below
# 225 us found the helper spinning (19 of 1290 asleep), those behind 250 us and more found it asleep (all 2570), so the range is centred
# there (150 .. 500 us gave 3008 sleeps and 999 hand-offs found awake).
PAUSE_US = (100.0, 450.0)


def test_paced_one_frame_calls_cross_the_helper_transition():
    """4000 calls behind pauses around the spin limit, 300 behind 2 ms pauses (the helper always asleep), 300 back to back (always awake):
    every call returns and equals the oracle (the child ends with status 4 otherwise), and the counters show the hand-offs meant."""
    child = os.path.join(ROOT, "tests", "one_frame_pauses_child.py")
    res = subprocess.run([sys.executable, child, str(CALLS), str(PAUSE_US[0]), str(PAUSE_US[1])], capture_output=True, text=True, cwd=ROOT, timeout=120)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    k = json.loads(res.stdout.strip().splitlines()[-1])
    paced, asleep, b2b = k["paced"], k["asleep"], k["back_to_back"]
    assert paced["jobs"] == CALLS and asleep["jobs"] == 300 and b2b["jobs"] == 300, k   # every call went through the helper
    assert paced["sleeps"] >= 400, k
    assert paced["awake"] >= 400, k
    assert asleep["sleeps"] >= 290, k
    assert b2b["sleeps"] <= 5, k


def test_one_frame_call_beyond_the_first_slice_of_records():
    """A one-frame call whose raw records exceed the first slice of 2048 that travels with the header: collect fetches the rest from the
    device slot, after the slot's event even when the header poll has already seen the call's sequence word."""
    W, H, thr = 320, 240, 45.0
    bank = synth.make_bank(40, seed=621, size_range=(30.0, 70.0))
    src = synth.make_scene(bank, W, H, seed=622)[0]
    ref = o.OracleDetector(bank).match(src, thr)
    det = Detector(bank, W, H, max_candidates=1 << 15)
    for _ in range(3):   # the second and third call find helper, queues and clocks awake: the poll is the likelier to see the word
        got = det.match(src, thr)
        assert det.stats()["raw_matches"] > 2048
        assert len(got) == len(ref)
        for f in ("x", "y", "similarity", "template_id", "class_index"):
            assert np.array_equal(got[f], ref[f]), f
    assert det.launch_helper_counters()["jobs"] == 3
    det.close()
