"""lmx_ctx_export_matches_on through Detector.export_matches: the final matches and clusters of an enqueue left in device memory.
The configuration is tests/test_gpu_chain_large_e2e.py's (160 x 160, bank seed 91, threshold 45, its side-car): frame A leaves more than
2048 raw records (the large-frame kernel), B fewer (the LDS kernel), Z none.  The reference is the CPU oracle (OracleDetector.match +
cluster_matches per frame, computed once in `cfg`), and the same enqueue through collect / collect_clusters afterwards; everything is
compared with array_equal.  Frames always arrive through upload_device from torch tensors.
Not reached: a frame beyond 16384 records (no small configuration makes one; tests/test_export_pack_host.py covers its status), and the
refusal of a device group's member context, which has no public handle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cluster_cases as cc
from linemod_pose_estimation_amd import Detector, ExportedMatches, PinnedArena, _lib, synth
from linemod_pose_estimation_amd import detector as D
from oracle import oracle as o

pytestmark = pytest.mark.gpu

S, THR, N_T = 160, 45.0, 80
SIDE = (10, 0.5, 0.1, 2)
CANARY = 0x5a5a5a5a


@pytest.fixture(scope="module")
def cfg():
    bank = synth.make_bank(N_T, seed=91, size_range=(20.0, 36.0))
    rng = np.random.default_rng(7)
    dists = 0.5 + 0.1 * (np.arange(N_T) % 4) + rng.uniform(-0.005, 0.005, N_T)
    rects = np.stack([np.zeros(N_T), np.zeros(N_T), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    frames = {"A": synth.make_scene(bank, S, S, seed=94)[0], "B": synth.make_scene(bank, S, S, seed=93, n_instances=1)[0],
              "Z": [np.full((S, S, 3), 90, np.uint8), np.full((S, S), 800, np.uint16)]}
    od = o.OracleDetector(bank)
    ref, raw, dev = {}, {}, {}
    for k, fr in frames.items():
        fr = [np.ascontiguousarray(s) for s in fr]
        m = od.match(fr, THR)
        raw[k] = len(od.last_raw())
        c, mem = o.cluster_matches(m, dists, rects, *SIDE) if len(m) else (np.zeros(0, D.CLUSTER_DTYPE), np.zeros(0, np.int32))
        ref[k] = (m, c, mem)
        dev[k] = [torch.from_numpy(fr[0]).cuda(), torch.from_numpy(fr[1].view(np.int16)).cuda()]
    # what the frames are chosen for
    assert cc.F2_MAX < raw["A"] <= 16384 and 0 < raw["B"] < cc.F2_MAX and raw["Z"] == 0, raw
    assert len(ref["A"][1]) > 0 and len(ref["B"][1]) > 0 and len(ref["Z"][0]) == 0
    det = Detector(bank, S, S, max_batch=3, max_candidates=1 << 17)
    det.set_cluster_sidecar(dists, rects, *SIDE)
    yield SimpleNamespace(bank=bank, dists=dists, rects=rects, ref=ref, raw=raw, dev=dev, det=det)
    det.close()


def n_members(ref):
    return int(ref[1]["member_count"].sum())


def totals(cfg, names):
    return (sum(len(cfg.ref[k][0]) for k in names), sum(len(cfg.ref[k][1]) for k in names), sum(n_members(cfg.ref[k]) for k in names))


def same_matches(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k in cc.FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k)


def same_as_oracle(got, ref, what, clusters=True, member_base=0):
    """one frame of to_host() against the oracle's (matches, clusters, members); the export's member_begin counts from the batch's start"""
    assert got is not None, what
    m, c, mem = got
    same_matches(m, ref[0], what)
    if not clusters:
        assert len(c) == 0 and len(mem) == 0
        return
    assert len(c) == len(ref[1]), (what, len(c), len(ref[1]))
    for k in ("index", "rect", "score", "member_count"):
        assert np.array_equal(c[k], ref[1][k]), (what, k)
    assert np.array_equal(c["member_begin"], ref[1]["member_begin"] + member_base), what
    for a, b in zip(c, ref[1]):
        assert np.array_equal(mem[a["member_begin"]:a["member_begin"] + a["member_count"]], ref[2][b["member_begin"]:b["member_begin"] + b["member_count"]]), what


def same_as_collect_clusters(host, collected, what):
    """to_host() against Detector.collect_clusters of the same enqueue: every field, member_begin and the flat member array included"""
    n_mem = 0
    for f, (got, (m, c, mem)) in enumerate(zip(host, collected)):
        same_matches(got[0], m, (what, f))
        assert len(got[1]) == len(c), (what, f)
        for k in cc.CLUSTER_FIELDS:
            assert np.array_equal(got[1][k], c[k]), (what, f, k)
        n_mem += int(c["member_count"].sum())
    assert np.array_equal(host[0][2][:n_mem], collected[0][2][:n_mem]) and len(host[0][2]) == n_mem, what


def upload_enqueue(cfg, names, det=None, stream=None):
    det = det or cfg.det
    det.upload_device([cfg.dev[k] for k in names], stream=stream)
    det.enqueue(len(names), THR)


def check_batch(cfg, res, names, clusters=True):
    """every frame delivered and the oracle's; offsets, raw_records and header as include/lmx.h lays them out"""
    host = res.to_host()
    info = res.frame_info.cpu().numpy()
    header = res.header.cpu().numpy()
    pos = [0, 0, 0]
    for f, k in enumerate(names):
        ref = cfg.ref[k]
        nc, nmem = (len(ref[1]), n_members(ref)) if clusters else (0, 0)
        assert info[f].tolist() == [pos[0], len(ref[0]), pos[1], nc, pos[2], nmem, 0, cfg.raw[k]], (f, k, info[f])
        same_as_oracle(host[f], ref, (f, k), clusters, pos[2])
        pos = [pos[0] + len(ref[0]), pos[1] + nc, pos[2] + nmem]
    assert header[:5].tolist() == [len(names), 0] + pos and header[6] == sum(cfg.raw[k] for k in names) and not header[7:].any(), header
    return host


# ---- 1. results ------------------------------------------------------------------------------------------------------------------------------

def test_batch_with_a_large_an_empty_and_a_small_frame(cfg):
    names = ["A", "Z", "B"]
    upload_enqueue(cfg, names)
    res = cfg.det.export_matches(3, clusters=True, max_large_frames=1)
    assert res.header.is_cuda and res.matches.shape == (1 << 16, 5) and res.clusters.shape == (4096, 48) and res.similarity.dtype == torch.float32
    host = check_batch(cfg, res, names)
    info = res.frame_info.cpu().numpy()
    assert info[:, 0].tolist() == [0, len(cfg.ref["A"][0]), len(cfg.ref["A"][0])] and info[:, 2].tolist() == [0, len(cfg.ref["A"][1]), len(cfg.ref["A"][1])]
    assert np.array_equal(res.similarity[:len(host[0][0])].cpu().numpy(), cfg.ref["A"][0]["similarity"])
    same_as_collect_clusters(host, cfg.det.collect_clusters(3, cap_total=1 << 17), "A Z B")      # the same enqueue, after the export
    # matches alone, against collect
    cfg.det.enqueue(3, THR)
    res = cfg.det.export_matches(3, max_large_frames=1)
    assert res.clusters is None and res.members is None
    host = check_batch(cfg, res, names, clusters=False)
    for f, m in enumerate(cfg.det.collect(3, cap_total=1 << 17)):
        same_matches(host[f][0], m, f)


def test_one_small_frame(cfg):
    upload_enqueue(cfg, ["B"])
    res = cfg.det.export_matches(1, clusters=True, max_large_frames=1)
    host = check_batch(cfg, res, ["B"])
    same_as_collect_clusters(host, cfg.det.collect_clusters(1), "B")


# ---- 2. capacities ---------------------------------------------------------------------------------------------------------------------------

def test_capacities(cfg):
    names = ["A", "Z", "B"]
    tm, tc, tmem = totals(cfg, names)
    a_m, a_c, a_mem = totals(cfg, ["A"])
    upload_enqueue(cfg, names)
    stream = torch.cuda.current_stream()

    def run(caps):
        buf = ExportedMatches(3, True, (tm + 8, tc + 8, tmem + 8), stream, 0)
        buf._backing["matches"].fill_(CANARY)
        buf._backing["clusters"].fill_(0x5a)
        buf._backing["members"].fill_(CANARY)
        res = cfg.det.export_matches(3, clusters=True, max_large_frames=1, cap_matches=caps[0], cap_clusters=caps[1], cap_members=caps[2], out=buf)
        assert res is buf
        stream.synchronize()
        hdr, info = res.header.cpu().numpy(), res.frame_info.cpu().numpy()
        assert hdr[2:5].tolist() == [tm, tc, tmem], hdr                                          # the true totals, whatever fitted
        m, c, mem = (buf._backing[k].cpu().numpy() for k in ("matches", "clusters", "members"))
        assert (m[caps[0]:] == CANARY).all() and (c[caps[1]:] == 0x5a).all() and (mem[caps[2]:] == CANARY).all()      # nothing behind a capacity
        return hdr, info, m, c, mem, res.to_host()

    # exactly the totals: everything is written
    hdr, info, m, c, mem, host = run((tm, tc, tmem))
    assert hdr[1] == 0 and info[:, 6].tolist() == [0, 0, 0]
    for f, k in enumerate(names):
        same_as_oracle(host[f], cfg.ref[k], k, True, info[f, 4])
    # one match short: B's matches stay unwritten, the rest is as before
    hdr, info, m, c, mem, host = run((tm - 1, tc, tmem))
    assert hdr[1] == 4 and info[:, 6].tolist() == [0, 0, 4] and host[2] is None
    same_as_oracle(host[0], cfg.ref["A"], "A")
    assert (m[a_m:] == CANARY).all() and info[2, :6].tolist() == [a_m, tm - a_m, a_c, tc - a_c, a_mem, tmem - a_mem]
    b_clusters = c[a_c:tc].copy().view(D.CLUSTER_DTYPE).reshape(-1)
    assert np.array_equal(b_clusters["score"], cfg.ref["B"][1]["score"]) and np.array_equal(b_clusters["member_begin"], cfg.ref["B"][1]["member_begin"] + a_mem)
    # one member short: B's clusters and members stay unwritten, its matches arrive
    hdr, info, m, c, mem, host = run((tm, tc, tmem - 1))
    assert hdr[1] == 4 and info[:, 6].tolist() == [0, 0, 8]
    assert (c[a_c:] == 0x5a).all() and (mem[a_mem:] == CANARY).all()
    same_matches(m[a_m:tm].copy().view(D.MATCH_DTYPE).reshape(-1), cfg.ref["B"][0], "B")
    # no room at all: the counts are still true
    hdr, info, m, c, mem, host = run((0, 0, 0))
    assert hdr[1] == 4 and info[:, 6].tolist() == [12, 12, 12] and host == [None] * 3
    assert info[:, 1].tolist() == [a_m, 0, tm - a_m] and info[:, 5].tolist() == [a_mem, 0, tmem - a_mem]
    cfg.det.release()


# ---- 3. large frames and the slots of a call ----------------------------------------------------------------------------------------------------

def test_two_large_frames_and_one_slot(cfg):
    names = ["A", "A"]
    upload_enqueue(cfg, names)
    res = cfg.det.export_matches(2, clusters=True, max_large_frames=1)
    host = res.to_host()
    info, hdr = res.frame_info.cpu().numpy(), res.header.cpu().numpy()
    same_as_oracle(host[0], cfg.ref["A"], "frame 0")
    a_m, a_c, a_mem = totals(cfg, ["A"])
    assert host[1] is None and info[1].tolist() == [a_m, 0, a_c, 0, a_mem, 0, 1, cfg.raw["A"]] and hdr[1] & 2 and hdr[2:5].tolist() == [a_m, a_c, a_mem]
    got = cfg.det.collect_clusters(2, cap_total=1 << 17)                  # the fallback: the same enqueue through the host path
    for f in range(2):
        m, c, mem = got[f]
        same_matches(m, cfg.ref["A"][0], f)
        assert np.array_equal(c["score"], cfg.ref["A"][1]["score"]) and np.array_equal(c["rect"], cfg.ref["A"][1]["rect"])
    cfg.det.enqueue(2, THR)
    res = cfg.det.export_matches(2, clusters=True, max_large_frames=0)
    assert res.to_host() == [None, None]
    info = res.frame_info.cpu().numpy()
    assert info[:, 6].tolist() == [1, 1] and info[:, 7].tolist() == [cfg.raw["A"]] * 2 and not info[:, :6].any() and res.header.cpu().numpy()[1] == 2
    res = cfg.det.export_matches(2, clusters=True, max_large_frames=2)
    check_batch(cfg, res, names)
    cfg.det.release()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------------------

def test_nothing_waits_for_the_device(cfg):
    names = ["A", "Z", "B"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.randn((2048, 2048), device="cuda")

    def step():
        upload_enqueue(cfg, names, stream=s)
        res = cfg.det.export_matches(3, clusters=True, max_large_frames=1, stream=s)
        return res, res.clone()

    res, kept = step()                                        # warm-up: the export's buffers, the allocator's blocks, the kernels' code
    s.synchronize()
    cfg.det.release()
    del res, kept

    def filler(n):
        with torch.cuda.stream(s):
            for _ in range(n):
                torch.mm(a, a)

    n, t0, t1 = 16, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        t0.record(s)
        filler(n)
        t1.record(s)
        s.synchronize()
        if t0.elapsed_time(t1) >= 50.0:
            break
        n *= 2
        assert n <= 1 << 16
    filler(n)
    res, kept = step()
    done = torch.cuda.Event()
    done.record(s)
    assert not done.query()                                   # upload_device, enqueue, export_matches and the clones returned with the filler still running
    s.synchronize()
    for f, k in enumerate(names):
        same_as_oracle(kept.to_host()[f], cfg.ref[k], k, True, int(kept.frame_info[f, 4]))
    cfg.det.release()


# ---- 5. pipelining ---------------------------------------------------------------------------------------------------------------------------------

def test_three_enqueues_exported_oldest_first(cfg):
    det = Detector(cfg.bank, S, S, max_batch=3, max_candidates=1 << 17, overlap=True)
    det.set_cluster_sidecar(cfg.dists, cfg.rects, *SIDE)
    batches = [["A", "Z", "B"], ["B", "Z", "B"], ["Z", "B", "A"]]
    s = torch.cuda.Stream()
    for names in batches:
        upload_enqueue(cfg, names, det=det, stream=s)
    kept, buf = [], None
    for names in batches:
        buf = det.export_matches(3, clusters=True, oldest=True, max_large_frames=1, stream=s, out=buf)     # one set of buffers, written three times
        kept.append(buf.clone())                              # the consumer: on the stream, no host wait
        det.release()
    s.synchronize()
    for names, res in zip(batches, kept):
        check_batch(cfg, res, names)
    det.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_enqueue_and_the_context_usable(cfg):
    det = Detector(cfg.bank, S, S, max_batch=2, max_candidates=1 << 17)
    L = _lib.lib()
    stream = torch.cuda.current_stream()
    buf = ExportedMatches(1, True, (1 << 12, 256, 1 << 12), stream, 0)
    t = buf._backing

    def desc(**kw):
        d = _lib.ExportDesc(C.sizeof(_lib.ExportDesc), 0, 0, 1, t["header"].data_ptr(), t["frame_info"].data_ptr(), t["matches"].data_ptr(), 1 << 12,
                            t["clusters"].data_ptr(), 256, t["members"].data_ptr(), 1 << 12)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(word, n_frames=1, stream_handle=None, **kw):
        d = desc(**kw)
        st = L.lmx_ctx_export_matches_on(det.h, n_frames, C.byref(d), int(stream.cuda_stream) if stream_handle is None else stream_handle)
        assert st == _lib.LMX_ERR_INVALID_ARG, (word, st)
        assert word in L.lmx_last_error().decode(), (word, L.lmx_last_error().decode())

    refused("nothing enqueued")
    det.upload_device([cfg.dev["B"]])
    det.enqueue(1, THR)
    refused("struct_size", struct_size=C.sizeof(_lib.ExportDesc) - 8)
    refused("n_frames", n_frames=2)
    for name in ("header", "frame_info", "matches"):
        refused("must not be null", **{name: None})
    refused("lmx_ctx_set_cluster_sidecar", clusters=1)                        # no side-car yet
    det.set_cluster_sidecar(cfg.dists, cfg.rects, *SIDE)
    refused("clusters_out", clusters=1, clusters_out=None)
    refused("members", clusters=1, members=None)
    refused("max_large_frames", max_large_frames=-1)
    host = np.zeros(1 << 12, D.MATCH_DTYPE)
    refused("matches is", matches=host.ctypes.data)                           # pageable host memory
    arena = PinnedArena(1 << 16)
    pinned = arena.put(np.zeros(4096, np.int32))
    refused("members is", clusters=1, members=pinned.ctypes.data)
    refused("header is", header=pinned.ctypes.data)
    refused("matches must be aligned", matches=t["matches"].data_ptr() + 2)
    refused("clusters_out must be aligned", clusters=1, clusters_out=t["clusters"].data_ptr() + 4)
    refused("frame_info must be aligned", frame_info=t["frame_info"].data_ptr() + 1)
    # a stream that is being captured: the capture is begun and ended here, nothing is replayed
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    side = torch.cuda.Stream()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(side.cuda_stream, 2) == 0                # hipStreamCaptureModeRelaxed
    try:
        refused("captured", stream_handle=int(side.cuda_stream))
    finally:
        assert hip.hipStreamEndCapture(side.cuda_stream, C.byref(graph)) == 0
        if graph.value:
            hip.hipGraphDestroy(graph)
    # the enqueue is still there, and whole
    res = det.export_matches(1, clusters=True, max_large_frames=1, out=buf)
    same_as_oracle(res.to_host()[0], cfg.ref["B"], "B after the refusals")
    same_matches(det.collect(1)[0], cfg.ref["B"][0], "collect after the refusals")
    del arena
    det.close()


# ---- clone() of every exported result ------------------------------------------------------------------------------------------------------------
CLONE_TENSORS = ("header", "frame_info", "matches", "clusters", "members", "diffs", "ndiffs", "cluster_class", "chain_header", "leaders", "rough", "member_group",
                 "poses", "checks", "keep")
CLONE_PLAIN = ("caps", "cap", "cap_members", "n_frames", "score", "with_clusters", "with_classes", "stream")
# caps = (cap_matches, cap_clusters, cap_members) -> the objects to copy: every optional tensor present, and where the class has optional ones, absent
CLONE_CASES = {
    "ExportedMatches": lambda caps, *on: [D.ExportedMatches(2, True, caps, *on), D.ExportedMatches(2, False, caps, *on)],
    "ExportedClusters": lambda caps, *on: [D.ExportedClusters(2, 2, True, caps, *on), D.ExportedClusters(2, 1, False, caps, *on), D.ExportedClusters(2, 0, False, caps, *on)],
    "ExportedPoses": lambda caps, *on: [D.ExportedPoses(max(caps[1], 1), *on)],
    "ExportedRoughPoses": lambda caps, *on: [D.ExportedRoughPoses(max(caps[1], 1), caps[2], *on)],
}


@pytest.mark.parametrize("name", sorted(CLONE_CASES))
def test_clone_copies_every_tensor_and_attribute(name):
    stream, dev = torch.cuda.Stream(), torch.cuda.current_device()
    for caps in ((3, 2, 5), (0, 0, 0)):         # zero capacities: the tensor keeps one element, the view of it is empty
        for src in CLONE_CASES[name](caps, stream, dev):
            what = (name, caps, sorted(src._backing))
            with torch.cuda.stream(stream):
                for i, t in enumerate(src._backing.values()):
                    t.view(torch.uint8).fill_(0x11 * (i + 1))
            cp = src.clone()
            stream.synchronize()
            assert type(cp) is type(src) and sorted(vars(cp)) == sorted(vars(src)), what
            for k in CLONE_PLAIN:
                assert hasattr(cp, k) == hasattr(src, k), (what, k)
                if hasattr(src, k):
                    assert getattr(cp, k) == getattr(src, k) and type(getattr(cp, k)) is type(getattr(src, k)), (what, k)
            assert list(cp._backing) == list(src._backing), what
            seen = 0
            for i, (k, t) in enumerate(cp._backing.items()):
                assert t.shape == src._backing[k].shape and t.dtype == src._backing[k].dtype and t.device == src._backing[k].device, (what, k)
                assert torch.equal(t, src._backing[k]) and bool((t.view(torch.uint8) == 0x11 * (i + 1)).all()), (what, k)
            for k in CLONE_TENSORS:
                assert hasattr(cp, k) == hasattr(src, k), (what, k)
                a, b = getattr(src, k, None), getattr(cp, k, None)
                assert (a is None) == (b is None), (what, k)
                if a is None:
                    continue
                seen += 1
                assert a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride(), (what, k)
                # each is its own object's tensor or a view of it (an empty view has no address to compare)
                assert (b is cp._backing[k] or b._base is cp._backing[k]) and (a is src._backing[k] or a._base is src._backing[k]), (what, k)
                assert a.numel() == 0 or (b.data_ptr() == cp._backing[k].data_ptr() and a.data_ptr() == src._backing[k].data_ptr()), (what, k)
                assert torch.equal(a, b), (what, k)
            assert seen == len(src._backing), what          # every tensor has its named view
            if hasattr(src, "matches"):
                assert src.similarity.dtype == torch.float32 and torch.equal(src.similarity.view(torch.int32), cp.similarity.view(torch.int32)), what
            else:
                assert not hasattr(cp, "similarity"), what
            theirs = {t.data_ptr() for t in src._backing.values()}
            assert 0 not in theirs and not theirs & {t.data_ptr() for t in cp._backing.values()}, what
            assert not theirs & {getattr(cp, k).data_ptr() for k in CLONE_TENSORS if getattr(cp, k, None) is not None}, what
            with torch.cuda.stream(stream):
                for t in src._backing.values():         # what is written to the original afterwards does not reach the copy
                    t.view(torch.uint8).fill_(0xEE)
            stream.synchronize()
            assert all(bool((t.view(torch.uint8) == 0x11 * (i + 1)).all()) for i, t in enumerate(cp._backing.values())), what
