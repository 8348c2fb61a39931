"""k_score_coarse_sb tests its exact pruning bound inside the blocks behind the first one (segments of whole groups, each with a
bound test that counts the block's later groups as at most 3 real features each).  A mid-block test may only drop what is provably
dead, so for every input the matches are those of the oracle and of the same context built with LMX_SCORE_NO_PRUNE=1 (no early
exit at all), as sets.  Shapes: the smallest that reach every path of the pass loop --
  1 x 640x480   1200 cells: templates with more than 1008 placements run a two-chunk pass and a one-chunk pass in the same wave
  9 x 640x480   XCD-aware frame placement (eight frames and more), ragged last group
  1 x 512x384   32 x 24 cells: one two-chunk pass whose second chunk is partly dead from the start
Banks: 62 coarsest-level features (five blocks, both modalities) and 17 of ColorGradient alone (a second block that is almost all
padding: its mid-block bounds undercount).  Thresholds 55, 80, 92 with planted instances, so candidates exist at each."""
import numpy as np
import pytest

from linemod_pose_estimation_amd import Detector, synth
from oracle import oracle as o

pytestmark = pytest.mark.gpu

THRESHOLDS = (55.0, 80.0, 92.0)
BANKS = {
    "rgbd_62": dict(modalities=("ColorGradient", "DepthNormal"), num_features=63, seed=901),   # 31 + 31 at the coarsest level
    "color_17": dict(modalities=("ColorGradient",), num_features=35, seed=902),                # 17
}
SHAPES = {"1x640x480": (1, 640, 480, 9100), "9x640x480": (9, 640, 480, 9200), "1x512x384": (1, 512, 384, 9300)}   # frames, W, H, first scene seed
_banks = {}


def bank_of(name):
    if name not in _banks:
        kw = BANKS[name]
        bank = synth.make_bank(48, T=(4, 8), size_range=(30.0, 70.0), **kw)
        _banks[name] = (bank, o.OracleDetector(bank))
    return _banks[name]


def as_set(m):
    return sorted(zip(*(m[k].tolist() for k in ("x", "y", "similarity", "template_id", "class_index"))))


def placements(bank, W, H):
    """Placements of every template on the coarsest level's grid of cells."""
    L, M, T = len(bank.T), len(bank.modalities), bank.T[-1]
    Wc, Hc = (W >> (L - 1)) // T, (H >> (L - 1)) // T
    rows = bank.classes[0][1].reshape(-1, L * M, 5)[:, (L - 1) * M]
    wf, hf = (rows[:, 0] - 1) // T + 1, (rows[:, 1] - 1) // T + 1
    return np.maximum(0, (Hc - hf) * Wc + (Wc - wf) + 1)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("bank_name", list(BANKS))
def test_segmented_bound_tests_keep_every_match(bank_name, shape, monkeypatch):
    n, W, H, seed0 = SHAPES[shape]
    bank, od = bank_of(bank_name)
    total = sum(max(1, m["num_features"] >> 1) for m in bank.modalities)
    assert total == {"rgbd_62": 62, "color_17": 17}[bank_name]
    pos = placements(bank, W, H)
    if (W, H) == (640, 480):
        assert (pos > 1008).any()                      # a two-chunk pass and then a one-chunk pass
    else:
        assert ((pos > 504) & (pos < 1008)).all()      # one two-chunk pass, second chunk partly dead
    frames = [synth.make_scene(bank, W, H, seed=seed0 + f)[0] for f in range(n)]
    det = Detector(bank, W, H, max_batch=n, max_candidates=1 << 18)
    monkeypatch.setenv("LMX_SCORE_NO_PRUNE", "1")      # read when the context is created
    full = Detector(bank, W, H, max_batch=n, max_candidates=1 << 18)
    monkeypatch.delenv("LMX_SCORE_NO_PRUNE", raising=False)
    assert det.device_kernel_name("k_score_coarse") == full.device_kernel_name("k_score_coarse") == "k_score_coarse_sb"
    det.upload(frames)
    full.upload(frames)
    for thr in THRESHOLDS:
        refs = [as_set(od.match(f, thr)) for f in frames]
        det.enqueue(n, thr)
        got = [as_set(g) for g in det.collect(n, cap_total=1 << 19)]
        assert det.stats()["candidates"] > 0
        full.enqueue(n, thr)
        got_full = [as_set(g) for g in full.collect(n, cap_total=1 << 19)]
        assert sum(len(r) for r in refs) > 0, thr
        for f in range(n):
            assert got[f] == refs[f], (thr, f)
            assert got[f] == got_full[f], (thr, f)
    det.close()
    full.close()
