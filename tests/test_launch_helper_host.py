"""The hand-off between lmx_match's calling thread and its helper thread (lmx::LaunchHelper, csrc/lmx_launch_helper.hpp), on the CPU: the
stress program tests/cpp/launch_helper_main.cpp built with g++ from that header alone and run as a plain child process.

What it is after is a LOST WAKE-UP: the helper spins for a bounded time behind a job and then sleeps on a condition variable; submit() wakes
it only if it reads `sleeping_`.  With release / acquire accesses the helper's store of sleeping_ could still sit in its store buffer when
it read the generation counter for the last time, the submitter then read sleeping_ == false and sent nothing, and lmx_match never came
back.  The program paces its submits around the spin limit so that they fall into that transition, checks every job's results, builds and
destroys 2000 helpers in every state, throws from a job, and ends with status 3 when a job is not done 5 s after its submit.

How many transitions a run must cross (N_MIN): against the class as it was before the fix (moved into its header, counters added, the four
accesses still release / acquire) the program lost a wake-up in every one of 40 runs on the machine this was written on, two series of ten
per spin limit (the first with gaps that reached 4 us further up); SLEEPS_UNTIL_LOSS holds the helper's sleep count when each run stopped.
The bound is 20 times the largest of them, for the sleeps and for the hand-offs that found the helper awake alike (counts, not shares):
the hit rate per transition varied by three orders of magnitude between runs.  At 300 us a job and its gap take 0.3 ms, so that run takes
about 100 s: the price of a bound that is 20 times a loss that once took 7074 sleeps to show.
The thread-sanitizer build runs the same program with fewer iterations: any report, or a status other than 0, fails."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "linemod_pose_estimation_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "launch_helper_main.cpp")
COMMON = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", CSRC]

# sleeps until the wake-up was lost, ten runs per spin limit, class before the fix (see the module docstring)
SLEEPS_UNTIL_LOSS = {
    20: (56, 220, 211, 396, 926, 230, 452, 317, 2491, 173,
         18, 40, 6, 381, 2171, 260, 1375, 293, 12, 11),
    300: (2745, 461, 3507, 5182, 167, 666, 937, 255, 7074, 293,
          1839, 563, 898, 1797, 2166, 3593, 2581, 248, 321, 677),
}
N_MIN = 20 * max(max(v) for v in SLEEPS_UNTIL_LOSS.values())   # 141 480
# iterations that reach N_MIN on both counts with room to spare: about half of the gaps end on either side of the transition (measured with
# the fix: 151 484 sleeps / 172 313 awake of 320 000 at 20 us, where 2 us are a tenth of the gaps' range, 160 994 / 159 524 at 300 us)
ITERATIONS = {20: 400000, 300: 320000}


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++"] + flags + COMMON + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory, "launch_helper_plain", ["-O2"])


@pytest.fixture(scope="module")
def tsan(tmp_path_factory):
    return _build(tmp_path_factory, "launch_helper_tsan", ["-O1", "-g", "-fsanitize=thread"])


def _run(exe, iterations, spin_us, seed, timeout):
    res = subprocess.run([exe, str(iterations), str(spin_us), str(seed)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = "\n".join(res.stdout.strip().splitlines()[-12:])
    print(tail)
    return res.returncode, res.stdout, tail


def _counters(last_line):
    return {k: int(v) for k, v in (kv.split("=") for kv in last_line.split())}


@pytest.mark.parametrize("spin_us", [300, 20])
def test_paced_submits_lose_no_wake_up(plain, spin_us):
    """Production's spin limit and one an order of magnitude shorter (as many more transitions per second): every job runs once and in order,
    no job waits 5 s, and the run crossed the spin-to-sleep transition at least N_MIN times from either side."""
    rc, out, tail = _run(plain, ITERATIONS[spin_us], spin_us, 1, 400)
    assert rc == 0, tail
    k = _counters(out.strip().splitlines()[-1])
    assert k["jobs"] == ITERATIONS[spin_us], tail
    assert k["sleeps"] >= N_MIN, (N_MIN, tail)
    assert k["awake"] >= N_MIN, (N_MIN, tail)


def test_back_to_back_submits_find_the_helper_awake(plain):
    """The hot path: a caller that comes straight back pays no wake-up.  The program's first phase submits 20 000 jobs with no gap: the next
    submit follows a job's end within a microsecond, against a spin limit of 20 us, so only a submitter that the scheduler took off its core
    for longer than that can find the helper asleep.  One in a hundred is allowed for that; a hand-off that notified every time would show
    20 000."""
    rc, out, tail = _run(plain, 20000, 20, 2, 60)
    assert rc == 0, tail
    line = [l for l in out.splitlines() if l.startswith("back to back: ")][-1]
    k = _counters(line[len("back to back: "):])
    assert k["jobs"] == 20000, tail
    assert k["notifies"] <= 200 and k["sleeps"] <= 200, tail


def test_thread_sanitizer_build(tsan):
    """The same program under -fsanitize=thread (a stand-alone program: nothing of it is loaded into Python): the 20 us limit, the lifetimes
    and the throwing job.  The job's plain stores into the submitter's frame are published by wait() alone."""
    rc, out, tail = _run(tsan, 20000, 20, 3, 300)
    assert rc == 0, tail
    assert "ThreadSanitizer" not in out and "WARNING" not in out, tail
    k = _counters(out.strip().splitlines()[-1])
    assert k["jobs"] == 20000 and k["sleeps"] >= 1000 and k["awake"] >= 1000, tail
