"""k_score_coarse_sb scores its template on several frames per wave (the frames k, k + 8, ... of one XCD slot, FPW at the most; the
launcher picks FPW from the batch size).  Whatever a wave keeps from one frame to the next must be the template's alone: accumulators and
live flags start afresh per frame.  So, for the default kernel, the full-work build (LMX_SCORE_NO_PRUNE=1) and the unchanged
k_score_coarse_u8, every frame's matches are the oracle's as a set, and the candidate count is the sum of the oracle's.  Shapes:
  640x480, 9 / 17 / 23 frames   ragged XCD groups and ragged frame groups for every FPW; templates of two and three chunks (a two-chunk
                                pass and a one-chunk pass per frame)
  320x240, 17 frames            every template is one chunk
  the 17-frame batches with frames 1, 8 and 10 blank (constant colour, constant depth): nothing there, the neighbours unchanged --
                                state carried from frame to frame would show here
  a two-class bank with one class excluded by class_ids: its waves leave before any frame
Thresholds 80 and 86.  The oracle's results per (scene, threshold) are computed once and shared."""
import numpy as np
import pytest

from linemod_pose_estimation_amd import Detector, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

THRESHOLDS = (80.0, 86.0)
BLANK = (1, 8, 10)
MODES = {"default": ({}, "k_score_coarse_sb"), "no_prune": ({"LMX_SCORE_NO_PRUNE": "1"}, "k_score_coarse_sb"), "u8": ({"LMX_SCORE_KERNEL": "u8"}, "k_score_coarse_u8")}
# bank arguments, frame size, scene seed of frame 0, scene arguments
SETS = {
    "640x480": (dict(n_templates=48, seed=77, size_range=(40.0, 300.0)), 640, 480, 500, {}),
    "320x240": (dict(n_templates=48, seed=78, size_range=(40.0, 110.0)), 320, 240, 700, dict(n_instances=3, n_distractors=2)),
    "two_classes": (dict(n_templates=32, seed=79, size_range=(40.0, 110.0), classes=["a", "b"]), 320, 240, 900, dict(n_instances=8, n_distractors=2)),
}
_banks, _scenes, _refs = {}, {}, {}


def bank_of(name):
    if name not in _banks:
        kw = dict(SETS[name][0])
        bank = synth.make_bank(kw.pop("n_templates"), **kw)
        _banks[name] = (bank, o.OracleDetector(bank))
    return _banks[name]


def scene(name, f):
    """Frame f of the set; f = -1 is the blank frame."""
    if (name, f) not in _scenes:
        bank, _ = bank_of(name)
        _, W, H, seed0, kw = SETS[name]
        if f < 0:
            _scenes[name, f] = [np.full((H, W, 3), 90, np.uint8), np.full((H, W), 1200, np.uint16)]
        else:
            _scenes[name, f] = synth.make_scene(bank, W, H, seed=seed0 + f, **kw)[0]
    return _scenes[name, f]


def as_set(m):
    return sorted(zip(*(m[k].tolist() for k in ("x", "y", "similarity", "template_id", "class_index"))))


def reference(name, f, thr, class_ids=()):
    """(matches as a sorted list, coarse candidates) of the oracle; never modified."""
    key = (name, f, thr, tuple(class_ids))
    if key not in _refs:
        _, od = bank_of(name)
        m = od.match(scene(name, f), thr, class_ids=class_ids)
        _refs[key] = (as_set(m), od.last_candidates())
    return _refs[key]


def chunks_per_template(bank, W, H):
    L, M, T = len(bank.T), len(bank.modalities), bank.T[-1]
    Wc, Hc = (W >> (L - 1)) // T, (H >> (L - 1)) // T
    rows = bank.classes[0][1].reshape(-1, L * M, 5)[:, (L - 1) * M]
    wf, hf = (rows[:, 0] - 1) // T + 1, (rows[:, 1] - 1) // T + 1
    return (np.maximum(0, (Hc - hf) * Wc + (Wc - wf) + 1) + 503) // 504


def run(name, indices, mode, monkeypatch, class_ids=()):
    env, kernel = MODES[mode]
    bank, _ = bank_of(name)
    _, W, H, _, _ = SETS[name]
    n = len(indices)
    frames = [scene(name, f) for f in indices]
    for k in ("LMX_SCORE_NO_PRUNE", "LMX_SCORE_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when the context is created
    det = Detector(bank, W, H, max_batch=n, max_candidates=1 << 18)
    assert det.device_kernel_name("k_score_coarse") == kernel
    det.upload(frames)
    for thr in THRESHOLDS:
        refs = [reference(name, f, thr, class_ids) for f in indices]
        det.enqueue(n, thr, class_ids=class_ids)
        got = [as_set(g) for g in det.collect(n, cap_total=1 << 19)]
        candidates = det.stats()["candidates"]
        print(name, mode, n, thr, "candidates", candidates, "oracle", sum(c for _, c in refs), "matches", [len(g) for g in got])
        assert candidates > 0
        assert candidates == sum(c for _, c in refs), thr
        for i, f in enumerate(indices):
            if f < 0:
                assert refs[i][0] == [] and got[i] == [], (thr, i)
            else:
                assert len(refs[i][0]) > 0, (thr, i)          # a condition on the inputs, met on the oracle alone
                assert got[i] == refs[i][0], (thr, i)
    det.close()


@pytest.mark.parametrize("n", (9, 17, 23))
@pytest.mark.parametrize("mode", list(MODES))
def test_ragged_batches_of_two_and_three_chunk_templates(mode, n, monkeypatch):
    bank, _ = bank_of("640x480")
    chunks = chunks_per_template(bank, 640, 480)
    assert (chunks == 2).sum() == 37 and (chunks == 3).sum() == 11
    run("640x480", list(range(n)), mode, monkeypatch)


@pytest.mark.parametrize("mode", list(MODES))
def test_one_chunk_templates(mode, monkeypatch):
    bank, _ = bank_of("320x240")
    assert (chunks_per_template(bank, 320, 240) == 1).all()
    run("320x240", list(range(17)), mode, monkeypatch)


@pytest.mark.parametrize("name", ("640x480", "320x240"))
@pytest.mark.parametrize("mode", list(MODES))
def test_blank_frames_between_busy_ones(mode, name, monkeypatch):
    run(name, [-1 if f in BLANK else f for f in range(17)], mode, monkeypatch)


@pytest.mark.parametrize("mode", list(MODES))
def test_a_disabled_class_leaves_before_any_frame(mode, monkeypatch):
    bank, _ = bank_of("two_classes")
    assert [c[0] for c in bank.classes] == ["a", "b"]
    run("two_classes", list(range(17)), mode, monkeypatch, class_ids=("b",))
    # and the whole bank on the same frames, so that the excluded class is known to have had something to say
    for thr in THRESHOLDS:
        assert sum(reference("two_classes", f, thr)[1] for f in range(17)) > sum(reference("two_classes", f, thr, ("b",))[1] for f in range(17))
