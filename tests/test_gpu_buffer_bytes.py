"""Every byte of the device's spread images and response memories, pads and tails included, against the expected blocks of np_restatement.py
(spread_block, nibble_block, byte_block: the layout of LevelGeom restated, filled with the CPU oracle's arrays), through the raw debug reads
(Detector.debug_raw).  k_refine and the scoring kernels read these pads as zeros, and the buffers are zeroed only when the context is
created: one stray byte of a writer stays for the life of the context.

After every collect of a sequence of calls on ONE context: every allocation equals the expected blocks for the frames of the batch, the
blocks of the frames beyond the batch equal what the previous call left there (zeros before the first), the 8192 bytes behind the last
block are zero, and the matches equal the oracle's.  first_difference names the place of the first wrong byte (own half, duplicate half,
wrapped duplicate, zero row, zero run, inter-orientation pad, block tail, tail).

Inputs reach the image borders (synth scenes do not): colour is the `smooth` generator of test_color_kernel_host, depth is planes in 16-px
facets around 1000 mm.  Depth labels are empty in the last cell row and column at small T (the quantiser's border, upstream's too), so the
edges are carried by a colour modality, which every modality slot holds in at least one case; each case asserts on the oracle's output that
the first and last cell row and cell column of every colour level are non-zero in at least half their bytes.

Shapes: the smallest that take each writer path (the case asserts the level-0 bands and whether byte-wide memories exist):
  T = (5, 8)     160 x 80    2 bands; level 1 has Wc = 10: the generic kernel (k_spread_linearize) writes byte-wide memories, k_pack_nibbles packs them
                 240 x 160   3 bands; level 1 is 120 x 80, Wc = 15: the generic kernel at an odd width, k_pack_nibbles
                 320 x 240   4 bands; level 1 has Wc = 20: the fast kernel writes byte-wide memories, k_pack_nibbles; once more with LMX_LS_FLAT
                 640 x 480   8 bands, one frame: nibbles written directly, both levels in one k_small_spread<5, 8> launch
                 80 x 160    flat level 0 (Wc = 16); level 1 has Wc = 5: the generic kernel
  T = (4, 8)     128 x 64, 256 x 192   2 and 4 bands; nibbles written directly, k_small_spread<4, 8> for one and two frames; 128 x 64 once more
                 with three modalities (no small chain: one launch per level, the nibble allocation holds [3][9] blocks)
  T = (4, 8, 10) 320 x 320   5 bands, a flat middle level (Wc = 20), the generic coarsest level (T = 10)
  T = (8,)       160 x 80    one level: no spread image at all
The small chain (one or two frames) exists for the banks (ColorGradient) and (ColorGradient, DepthNormal) only.
Calls (max_batch = 9): 9 frames (the XCD placement with a ragged second group of eight), 1 (the small chain, fused where the level pair has a
kernel), 2, 3 (the plain grid), 1 masked frame (the plain chain), 9 again; a hipGraph context replays 3 and 9 frames twice each; an overlap
context has two enqueues in flight."""
import numpy as np
import pytest

import np_restatement as R
from linemod_pose_estimation_amd import Detector, _lib, synth
from oracle import oracle as o
from test_buffer_layout_host import geometry_of
from test_color_kernel_host import image

pytestmark = pytest.mark.gpu

THR = 60.0
CG, DN = "ColorGradient", "DepthNormal"
# id: T, W, H, modalities, LMX_LS_FLAT, bands of level 0, byte-wide coarsest memories, max_batch
CASES = {
    "160x80": ((5, 8), 160, 80, (CG, DN), False, 2, True, 9),
    "240x160": ((5, 8), 240, 160, (DN, CG), False, 3, True, 9),
    "320x240": ((5, 8), 320, 240, (CG,), False, 4, True, 9),
    "640x480": ((5, 8), 640, 480, (CG, DN), False, 8, False, 1),
    "128x64": ((4, 8), 128, 64, (CG, DN), False, 2, False, 9),
    "128x64_three_modalities": ((4, 8), 128, 64, (CG, DN, CG), False, 2, False, 9),
    "256x192": ((4, 8), 256, 192, (CG, DN), False, 4, False, 9),
    "80x160": ((5, 8), 80, 160, (DN, CG), False, 0, True, 9),
    "320x240_ls_flat": ((5, 8), 320, 240, (CG, DN), True, 0, True, 9),
    "320x320": ((4, 8, 10), 320, 320, (CG, DN, CG), False, 5, True, 9),
    "160x80_one_level": ((8,), 160, 80, (CG, DN), False, None, True, 9),
}
FUSED = ("640x480", "128x64", "256x192")   # a one- or two-frame call takes the small chain and its level pair has a k_small_spread kernel


def same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for k in ("x", "y", "similarity", "template_id", "class_index"):
        assert np.array_equal(a[k], b[k]), k


def depth_facets(rng, H, W):
    """Planes in 16-px facets around 1000 mm: normals of every direction, steps between the facets, nothing far or missing."""
    fy, fx = (H + 15) // 16, (W + 15) // 16
    a, b, c = (np.kron(rng.uniform(lo, hi, (fy, fx)), np.ones((16, 16)))[:H, :W] for lo, hi in ((-3, 3), (-3, 3), (-25, 25)))
    y, x = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(np.rint(1000 + c + a * (x % 16 - 8) + b * (y % 16 - 8)).astype(np.uint16))


class Case:
    """A bank, a pool of frames that reach the borders, and per pool frame the expected blocks and matches (computed once, on the CPU)."""

    def __init__(self, key, seed=0):
        self.T, self.W, self.H, self.mods, self.ls_flat, self.bands, self.byte_wide, self.max_batch = CASES[key]
        self.L, self.M = len(self.T), len(self.mods)
        self.bank = synth.make_bank(8, modalities=self.mods, T=self.T, seed=2100 + self.W + seed, num_features=63 // self.M,
                                    size_range=(16.0, min(self.W, self.H) * 0.45))
        self.od = o.OracleDetector(self.bank)
        rng = np.random.default_rng([self.W, self.H, seed])
        self.pool = [[image(rng, self.H, self.W, "smooth") if m == CG else depth_facets(rng, self.H, self.W) for m in self.mods] for _ in range(self.max_batch + 2)]
        self.masks = [np.ascontiguousarray(np.kron((rng.uniform(0, 1, (self.H // 4, self.W // 4)) < 0.8) * rng.integers(1, 256, (self.H // 4, self.W // 4)),
                                                   np.ones((4, 4))).astype(np.uint8)) for _ in self.mods]
        self._expected, self.n_candidates = {}, 0
        self.border_fractions = {}   # (level, modality) -> the smallest non-zero fraction of a first / last cell row / column over the pool

    def geometry(self, native):
        geom, _ = geometry_of(native, self.W, self.H, self.max_batch, self.ls_flat)
        return geom

    def expected(self, geom, p, masked=False):
        """Pool frame p -> {"ref": matches, ("ls", l, m) / ("nib", m) / ("lm", m): (bytes, kinds) of its block}."""
        if (p, masked) in self._expected:
            return self._expected[p, masked]
        e = {"ref": self.od.match(self.pool[p], THR, masks=self.masks if masked else None)}
        self.n_candidates += self.od.last_candidates()
        for l, g in enumerate(geom):
            for m in range(self.M):
                q = self.od.quantized(l, m, (g["H"], g["W"]))
                flat = o.linearize(o.spread(q, g["T"]), g["T"])
                if l < self.L - 1:
                    e["ls", l, m] = R.spread_block(g, flat)
                else:
                    lm = self.od.linear_memory(l, m, (g["H"], g["W"]))
                    e["nib", m] = R.nibble_block(g, lm)
                    if self.byte_wide:
                        e["lm", m] = R.byte_block(g, lm)
                if self.mods[m] == CG and not masked:   # the border condition, on the oracle's output alone
                    cells = (flat != 0).reshape(g["T"] ** 2, g["Hc"], g["Wc"])
                    worst = min(cells[:, 0, :].mean(), cells[:, -1, :].mean(), cells[:, :, 0].mean(), cells[:, :, -1].mean())
                    self.border_fractions[l, m] = min(self.border_fractions.get((l, m), 1.0), float(worst))
        self._expected[p, masked] = e
        return e


def allocations(case, geom):
    """key -> (what, level, modality, block stride, blocks) of every raw allocation of the context."""
    gc, F = geom[-1], case.max_batch
    out = {("nib",): (_lib.LMX_DBG_RAW_NIBBLES, 0, 0, gc["nib_mod_stride"], case.M * F)}
    for m in range(case.M):
        for l in range(case.L - 1):
            out["ls", l, m] = (_lib.LMX_DBG_RAW_SPREAD, l, m, geom[l]["ls_stride"], F)
        if case.byte_wide:
            out["lm", m] = (_lib.LMX_DBG_RAW_BYTES, case.L - 1, m, gc["mod_stride"], F)
    return out


def check_allocations(det, case, geom, batch, state, where):
    """batch: the expected dicts of the call's frames.  state: key -> the allocation as the previous call left it (updated)."""
    F = case.max_batch
    for key, (what, l, m, stride, n_blocks) in allocations(case, geom).items():
        got = det.debug_raw(what, n_blocks * stride + R.ALLOC_TAIL, l, m)
        prev = state.get(key)
        if prev is None:   # as the context's creation left it
            prev = np.zeros(len(got), np.uint8)
        blocks = []
        for b in range(n_blocks):
            f, ekey = (b % F, ("nib", b // F)) if key == ("nib",) else (b, key)
            kind = case.expected(geom, 0)[ekey][1]
            blocks.append(batch[f][ekey] if f < len(batch) else (prev[b * stride:(b + 1) * stride], kind))
        want, kind = R.allocation(blocks)
        diff = R.first_difference(got, want, kind)
        assert diff is None, (where, key, "block %d" % (diff[1] // stride), "in the batch" if diff[1] // stride % F < len(batch) else "beyond the batch", diff)
        state[key] = got


def run_call(det, case, geom, pool_ids, state, where, masked=False):
    frames = [case.pool[p] for p in pool_ids]
    det.upload(frames)
    if masked:
        det.upload_masks([case.masks] * len(frames))
    det.enqueue(len(frames), THR)
    got = det.collect(len(frames))
    batch = [case.expected(geom, p, masked) for p in pool_ids]
    check_allocations(det, case, geom, batch, state, where)
    for f, e in enumerate(batch):
        same(got[f], e["ref"])
    return sum(len(e["ref"]) for e in batch)


def open_context(case, monkeypatch, **kw):
    if case.ls_flat:
        monkeypatch.setenv("LMX_LS_FLAT", "1")
    det = Detector(case.bank, case.W, case.H, max_batch=case.max_batch, max_candidates=1 << 18, **kw)
    geom = case.geometry(det.native_bank)
    # the writer path the case is about: the level-0 form, and whether the spread kernel writes the nibbles itself
    assert case.bands is None or geom[0]["ls_bands"] == case.bands
    gc = geom[-1]
    if case.byte_wide:
        det.debug_raw(_lib.LMX_DBG_RAW_BYTES, case.max_batch * gc["mod_stride"] + R.ALLOC_TAIL, case.L - 1, 0)
    else:
        with pytest.raises(_lib.LmxError, match="writes the nibbles itself"):
            det.debug_raw(_lib.LMX_DBG_RAW_BYTES, case.max_batch * gc["mod_stride"] + R.ALLOC_TAIL, case.L - 1, 0)
    return det, geom


def check_borders(case):
    """First and last cell row and cell column of every colour level: non-zero in at least half their bytes, in every frame of the pool."""
    print("smallest non-zero fraction of a border cell row / column per (level, modality):", {k: round(v, 3) for k, v in sorted(case.border_fractions.items())})
    assert case.border_fractions and all(v >= 0.5 for v in case.border_fractions.values()), case.border_fractions


@pytest.mark.parametrize("key", list(CASES))
def test_every_byte_after_every_call(key, monkeypatch):
    case = Case(key)
    det, geom = open_context(case, monkeypatch)
    F, state, n_matches = case.max_batch, {}, 0
    # (frames of the pool, masked): every call brings frames the blocks it writes did not hold before
    calls = [(range(0, 9), False), ([9], False), ([10, 3], False), ([5, 6, 7], False), ([2], True), (range(2, 11), False)] if F == 9 else [([0], False), ([1], True), ([2], False)]
    for i, (ids, masked) in enumerate(calls):
        n_matches += run_call(det, case, geom, list(ids), state, "call %d: %d frame(s)%s" % (i, len(ids), ", masked" if masked else ""), masked)
    # the writer path, observed: launches per call with profiling on (the calls are checked like the others).  k_pack_nibbles runs once per
    # modality exactly where byte-wide memories exist; a one-frame call of a FUSED case spreads both levels in its one k_small_spread launch
    det.set_profiling(True)
    for n in sorted({1, F}):
        det.reset_profiling()
        run_call(det, case, geom, list(range(n)), state, "profiled call of %d frame(s)" % n)
        launches = {k: v[1] for k, v in det.kernel_times().items()}
        assert launches["k_pack_nibbles"] == (case.M if case.byte_wide else 0), (n, launches)
        if n == 1:
            assert (launches["k_spread_linearize"] == 1) == (key in FUSED or case.L == 1), launches
    det.close()
    check_borders(case)
    # the templates hardly fit the smallest shapes: there the refinement still gathers its patches for every candidate, but none passes
    assert case.n_candidates > 100 and (n_matches > 0 or min(case.W, case.H) <= 100), (case.n_candidates, n_matches)


def test_every_byte_when_a_graph_is_replayed(monkeypatch):
    case = Case("160x80", seed=1)
    det, geom = open_context(case, monkeypatch, hipgraph=True)
    state = {}
    for i, ids in enumerate(([0, 1, 2], [3, 4, 5], range(0, 9), range(2, 11), [6, 7, 8])):
        run_call(det, case, geom, list(ids), state, "graph call %d" % i)
    det.close()
    check_borders(case)


def test_every_byte_with_two_enqueues_in_flight(monkeypatch):
    """overlap=True: the second enqueue runs on the other lane's buffers; the raw reads return the lane of the most recent enqueue."""
    case = Case("160x80", seed=2)
    case.max_batch = 3
    det, geom = open_context(case, monkeypatch, overlap=True)
    for rnd, (a, b) in enumerate((([0, 1, 2], [3, 4, 0]), ([4, 2, 1], [1, 0, 3]))):
        det.upload([case.pool[p] for p in a])
        det.enqueue(3, THR)
        det.upload([case.pool[p] for p in b])
        det.enqueue(3, THR)
        first, second = det.collect(3), det.collect(3)
        check_allocations(det, case, geom, [case.expected(geom, p) for p in b], {}, "overlap round %d" % rnd)
        for f in range(3):
            same(first[f], case.expected(geom, a[f])["ref"])
            same(second[f], case.expected(geom, b[f])["ref"])
    det.close()
    check_borders(case)


def test_raw_reads_refuse_what_they_cannot_give(monkeypatch):
    case = Case("160x80", seed=3)
    det, geom = open_context(case, monkeypatch)
    g0, gc, F = geom[0], geom[1], case.max_batch
    n = F * g0["ls_stride"] + R.ALLOC_TAIL
    out = np.zeros(n, np.uint8)
    read = lambda frame, what, level, modality, nbytes: _lib.lib().lmx_ctx_debug_read(det.h, frame, what, level, modality, out.ctypes.data, nbytes)
    assert read(0, _lib.LMX_DBG_RAW_SPREAD, 0, 1, n) == _lib.LMX_OK and not out.any()      # a fresh context: zeros, pads and all
    assert read(1, _lib.LMX_DBG_RAW_SPREAD, 0, 0, n) == _lib.LMX_ERR_INVALID_ARG           # every frame comes at once
    assert read(0, _lib.LMX_DBG_RAW_SPREAD, 1, 0, n) == _lib.LMX_ERR_INVALID_ARG           # the coarsest level keeps no spread image
    with pytest.raises(_lib.LmxError, match=str(n)):
        det.debug_raw(_lib.LMX_DBG_RAW_SPREAD, n - 1, 0, 0)
    with pytest.raises(_lib.LmxError, match=str(case.M * F * gc["nib_mod_stride"] + R.ALLOC_TAIL)):
        det.debug_raw(_lib.LMX_DBG_RAW_NIBBLES, 16)
    with pytest.raises(_lib.LmxError, match=str(F * gc["mod_stride"] + R.ALLOC_TAIL)):
        det.debug_raw(_lib.LMX_DBG_RAW_BYTES, 16, 1, 1)
    det.close()
