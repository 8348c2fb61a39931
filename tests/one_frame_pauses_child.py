"""The child process of tests/test_gpu_one_frame_pauses.py: one-frame Detector.match calls on one context with busy-waited pauses between them,
every result compared with the oracle's, the helper thread's counters (Detector.launch_helper_counters) read around each loop.  Run on its own
so that a hand-off that hangs is the parent's timeout and not a stuck suite.
    usage: python one_frame_pauses_child.py CALLS PAUSE_LO_US PAUSE_HI_US [hist]
Prints one JSON line: the counters' increase over the paced loop, the 2 ms loop and the back-to-back loop.  With `hist`: per 25 us of pause,
how many of the calls behind such a pause found the helper asleep (for choosing the pause range on another machine)."""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linemod_pose_estimation_amd import Detector, synth  # noqa: E402
from oracle import oracle as o  # noqa: E402

W, H, THRESHOLD = 320, 240, 80.0
FIELDS = ("x", "y", "similarity", "template_id", "class_index")


def busy_wait(seconds):
    until = time.perf_counter() + seconds
    while time.perf_counter() < until:
        pass


def main():
    calls, lo_us, hi_us = int(sys.argv[1]), float(sys.argv[2]), float(sys.argv[3])
    hist = len(sys.argv) > 4 and sys.argv[4] == "hist"
    bank = synth.make_bank(40, seed=621, size_range=(30.0, 70.0))   # ColorGradient + DepthNormal, T = (5, 8)
    frames = [synth.make_scene(bank, W, H, seed=622 + f)[0] for f in range(5)]
    od = o.OracleDetector(bank)
    refs = [od.match(fr, THRESHOLD) for fr in frames]   # once
    assert all(len(r) > 0 for r in refs), [len(r) for r in refs]
    det = Detector(bank, W, H)
    zero = det.launch_helper_counters()
    assert zero == {"jobs": 0, "sleeps": 0, "notifies": 0, "awake": 0}, zero   # no helper before the first one-frame call

    def call(i):
        got, ref = det.match(frames[i % 5], THRESHOLD), refs[i % 5]
        if len(got) != len(ref) or not all(np.array_equal(got[k], ref[k]) for k in FIELDS):
            print("call %d: the matches differ from the oracle's (%d against %d)" % (i, len(got), len(ref)), flush=True)
            sys.exit(4)

    def loop(n, pause):
        """n calls, pause() seconds of busy-wait behind each -> the counters' increase, [(pause, the helper slept in it)]"""
        before, seen, slept = det.launch_helper_counters(), [], det.launch_helper_counters()["sleeps"]
        for i in range(n):
            call(i)
            p = pause()
            if p > 0.0:
                busy_wait(p)
            if hist:
                s = det.launch_helper_counters()["sleeps"]
                seen.append((p, s != slept))
                slept = s
        after = det.launch_helper_counters()
        return {k: after[k] - before[k] for k in after}, seen

    rng = random.Random(5)
    call(0)   # the first call creates the helper (and pays the first launches): not part of any count
    out = {}
    out["paced"], seen = loop(calls, lambda: rng.uniform(lo_us, hi_us) * 1e-6)
    out["asleep"], _ = loop(300, lambda: 2e-3)
    out["back_to_back"], _ = loop(300, lambda: 0.0)
    det.close()
    if hist:
        bins = {}
        for p, s in seen:
            b = bins.setdefault(int(p * 1e6 // 25) * 25, [0, 0])
            b[0] += 1
            b[1] += s
        out["hist_us_calls_slept"] = [[k, v[0], v[1]] for k, v in sorted(bins.items())]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
