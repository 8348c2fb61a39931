"""Gray colour sources on the device (LMX_CTX_GRAY, Detector(..., gray=True)): a MONO8 frame g is matched without the node's mixChannels,
on the one-plane colour kernels, and every stage equals the oracle run on bgr = g copied into B, G and R -- labels, linear memories,
the colour pyramid (channel 0), candidate counts and the final list in its order -- through every path the BGR context offers: batches,
hipGraph + device lanes, zero-copy pinned input, masks, the raw MONO8 upload with the node-side blur and crop, the one-frame streamed
call, template-shard groups, the cluster chain, the trainer and the cv::linemod facade.  Reference caller: the Ensenso nodes
(src/linemod_ensenso_detect_3_mult_detect_service.cpp:293-297 turn the MONO8 frame into BGR before match())."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from linemod_pose_estimation_amd import Detector, NativeBank, _lib, synth
from linemod_pose_estimation_amd.bank import DEFAULT_COLOR_GRADIENT, DEFAULT_DEPTH_NORMAL
from oracle import oracle as o

pytestmark = pytest.mark.gpu


def same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for k in ("x", "y", "similarity", "template_id", "class_index"):
        assert np.array_equal(a[k], b[k]), k


def rep3(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g)[..., None], 3, axis=2))


def gray_of(frame, row_pad=0):
    """A scene's colour source as a MONO8 frame (its green channel, like bench.py's raw camera frames), optionally as an ROI view with
    row padding; -> (gray sources, the same scene with the gray frame copied into B, G, R)."""
    g = np.ascontiguousarray(np.asarray(frame[0])[:, :, 1])
    if row_pad:
        H, W = g.shape
        wide = np.zeros((H, W + row_pad), np.uint8)
        wide[:, :W] = g
        g = wide[:, :W]
    return [g] + list(frame[1:]), [rep3(g)] + list(frame[1:])


CASES = [   # the CASES of test_gpu_parity.py that have ColorGradient
    # W, H, n, modalities, T, thr, size_range, row_pad
    (160, 160, 10, ("ColorGradient",), (5, 8), 70.0, (20.0, 36.0), 0),
    (160, 160, 10, ("ColorGradient", "DepthNormal"), (5, 8), 72.0, (20.0, 36.0), 24),
    (320, 240, 80, ("ColorGradient", "DepthNormal"), (5, 8), 80.0, (30.0, 80.0), 112),
    (640, 480, 200, ("ColorGradient",), (5, 8), 88.0, (55.0, 194.0), 112),
    (640, 480, 200, ("ColorGradient", "DepthNormal"), (5, 8), 85.0, (55.0, 194.0), 0),
    (256, 192, 30, ("ColorGradient", "DepthNormal"), (4, 8), 75.0, (24.0, 60.0), 0),
    (240, 240, 20, ("ColorGradient",), (5,), 75.0, (24.0, 60.0), 0),
    (480, 480, 20, ("ColorGradient", "DepthNormal"), (5, 8, 10), 70.0, (40.0, 100.0), 0),
]


@pytest.mark.parametrize("W,H,n,mods,T,thr,size_range,row_pad", CASES)
def test_gray_stagewise_and_final_parity(W, H, n, mods, T, thr, size_range, row_pad):
    bank = synth.make_bank(n, modalities=mods, T=T, seed=41, size_range=size_range)
    frame, _ = synth.make_scene(bank, W, H, seed=42, row_pad=0)
    gsrc, bsrc = gray_of(frame, row_pad)
    od = o.OracleDetector(bank)
    ref = od.match(bsrc, thr)
    det = Detector(bank, W, H, gray=True)
    got = det.match(gsrc, thr)
    L, M = len(T), len(mods)
    for l in range(L):
        for m in range(M):
            assert np.array_equal(det.debug_quantized(0, l, m), od.quantized(l, m, (H >> l, W >> l))), ("quant", l, m)
            assert np.array_equal(det.debug_linear_memory(0, l, m), od.linear_memory(l, m, (H >> l, W >> l))), ("lm", l, m)
    cg = mods.index("ColorGradient")
    pyr = bsrc[cg]
    for l in range(L):
        lv = det.debug_pyramid_bgr(0, l, cg)
        assert lv.shape == (H >> l, W >> l)
        assert np.array_equal(lv, pyr[..., 0]), l
        pyr = o.pyrdown(pyr)
    assert det.stats()["candidates"] == od.last_candidates()
    assert det.stats()["raw_matches"] == len(od.last_raw())
    same(got, ref)
    det.close()


def test_gray_batches_hipgraph_lanes_and_async_input():
    """Batches of 64 frames; hipGraph replay on device lanes; LMX_CTX_ASYNC_INPUT pulling pinned gray frames in place."""
    W, H = 320, 240
    bank = synth.make_bank(60, modalities=("ColorGradient", "DepthNormal"), seed=65, size_range=(30.0, 80.0))
    scenes = [synth.make_scene(bank, W, H, seed=660 + f)[0] for f in range(8)]
    pairs = [gray_of(s) for s in scenes]
    od = o.OracleDetector(bank)
    refs = [od.match(b, 78.0) for _, b in pairs]
    assert sum(len(r) for r in refs) > 8
    frames = [pairs[f % 8][0] for f in range(64)]
    for kw in (dict(), dict(hipgraph=True, overlap=True)):
        det = Detector(bank, W, H, max_batch=64, gray=True, **kw)
        det.upload(frames)
        for _ in range(3):                     # both output slots, lanes in turn, graphs replayed
            det.enqueue(64, 78.0)
            det.enqueue(64, 78.0)
            for outs in (det.collect(64), det.collect(64)):
                for f in range(64):
                    same(outs[f], refs[f % 8])
        det.close()
    # pinned frames, pulled by the device while the call returns
    from linemod_pose_estimation_amd.detector import PinnedArena
    det = Detector(bank, W, H, max_batch=4, gray=True, async_input=True)
    pp = PinnedArena(4 * (W * H + W * H * 2) + 4096)
    pinned = [[pp.put(g), pp.put(d)] for g, d in (pairs[f][0] for f in range(4))]
    for _ in range(2):
        det.upload(pinned)
        det.upload_wait()
        det.enqueue(4, 78.0)
        outs = det.collect(4)
        for f in range(4):
            same(outs[f], refs[f])
    det.close()
    pp.close()


def test_gray_masks():
    W, H = 320, 240
    bank = synth.make_bank(40, seed=301, size_range=(30.0, 70.0))
    od = o.OracleDetector(bank)
    det = Detector(bank, W, H, max_batch=3, gray=True)
    rng = np.random.default_rng(9)

    def blocky(p):
        m = (rng.uniform(0, 1, (H // 16, W // 16)) < p).astype(np.uint8) * rng.integers(1, 255, (H // 16, W // 16), dtype=np.uint8)
        return np.ascontiguousarray(np.kron(m, np.ones((16, 16), np.uint8)))
    pairs = [gray_of(synth.make_scene(bank, W, H, seed=302 + f)[0]) for f in range(3)]
    for case in range(3):
        masks = [blocky(0.7), blocky(0.8) if case != 1 else None]
        g, b = pairs[case]
        same(det.match_masked(g, masks, 72.0), od.match(b, 72.0, masks=masks))
        for l in range(2):
            for m in range(2):
                assert np.array_equal(det.debug_quantized(0, l, m), od.quantized(l, m, (H >> l, W >> l))), (case, l, m)
    bm = [[blocky(0.7), blocky(0.7)], [None, None], [blocky(0.6), None]]
    det.upload([p[0] for p in pairs])
    det.upload_masks(bm)
    det.enqueue(3, 72.0)
    outs = det.collect(3)
    for f in range(3):
        same(outs[f], od.match(pairs[f][1], 72.0, masks=None if f == 1 else bm[f]))
    det.close()


def test_gray_upload_raw_mono_752x480():
    """The Ensenso's raw MONO8 752x480 frame (+ float-metre depth) -> 3x3 blur on the full frame + crop (56, 0) on the device, into the
    one-byte level-0 frame: equal to the oracle's restatement of the node's steps (o.pre_color), channel 0, then the oracle's matches."""
    W, H, SW, SH, bias_x = 640, 480, 752, 480, 56
    bank = synth.make_bank(150, seed=63)
    det = Detector(bank, W, H, max_batch=2, gray=True)
    od = o.OracleDetector(bank)
    raw_frames, ref_sources = [], []
    for f in range(2):
        (bgr, depth), _ = synth.make_scene(bank, SW, SH, seed=64 + f, texture=0.8)
        mono = np.ascontiguousarray(bgr[:, :, 1])
        z = depth.astype(np.float32) / np.float32(1000.0)
        z[depth == 0] = np.nan
        raw_frames.append([mono, z])
        ref_sources.append([o.pre_color(mono, (bias_x, 0), (W, H), True), o.pre_depth(z, (bias_x, 0), (W, H))])
    for blur in (True, False):
        if not blur:
            ref_sources = [[o.pre_color(r[0], (bias_x, 0), (W, H), False), s[1]] for r, s in zip(raw_frames, ref_sources)]
        det.upload_raw(raw_frames, (SW, SH), (bias_x, 0), blur3=blur, mono=True, depth_float_m=True)
        det.enqueue(2, 85.0)
        outs = det.collect(2)
        for f in range(2):
            pre = ref_sources[f][0]
            assert pre.shape == (H, W, 3)
            assert np.array_equal(det.debug_pyramid_bgr(f, 0, 0), pre[..., 0])
            ref = od.match(ref_sources[f], 85.0)
            assert len(ref) > 0
            same(outs[f], ref)
    det.close()


def test_gray_one_frame_streamed_call(monkeypatch):
    """lmx_match with fresh host frames: the level-0 quantisers wait for the rows the caller is still storing (one byte per pixel now);
    streamed and store-then-launch agree with the oracle, ColorGradient only and RGB-D, many calls in a row, two-frame batches."""
    W, H = 640, 480
    for mods in (("ColorGradient", "DepthNormal"), ("ColorGradient",)):
        bank = synth.make_bank(120, modalities=mods, seed=611, size_range=(55.0, 150.0))
        od = o.OracleDetector(bank)
        pairs = [gray_of(synth.make_scene(bank, W, H, seed=612 + f)[0], row_pad=112 if f % 2 else 0) for f in range(5)]
        refs = [od.match(b, 86.0) for _, b in pairs]
        assert sum(len(r) for r in refs) > 5
        dets = {}
        for name, env in (("streamed", None), ("stored", "1")):
            if env:
                monkeypatch.setenv("LMX_NO_STREAM_STORE", env)
            dets[name] = Detector(bank, W, H, max_batch=2, gray=True)
            monkeypatch.delenv("LMX_NO_STREAM_STORE", raising=False)
        for _ in range(3):
            for f, (g, _) in enumerate(pairs):
                for det in dets.values():
                    same(det.match([np.array(s, copy=True) for s in g], 86.0), refs[f])   # a fresh frame every call
        for det in dets.values():
            got = det.match_batch([pairs[1][0], pairs[4][0]], 86.0)
            same(got[0], refs[1])
            same(got[1], refs[4])
            det.close()


def test_gray_template_shard_group_peer_copy():
    from linemod_pose_estimation_amd.dist import DeviceGroup
    W, H = 320, 240
    bank = synth.make_bank(40, seed=371, size_range=(30.0, 70.0))
    pairs = [gray_of(synth.make_scene(bank, W, H, seed=372 + f)[0]) for f in range(2)]
    od = o.OracleDetector(bank)
    g = DeviceGroup(bank, W, H, 2, devices=[0, 0], max_batch=2, collective="peer_copy", gray=True)
    for _ in range(2):
        g.upload([p[0] for p in pairs])
        g.submit(2, 78.0)
        got = g.finish(2)
        for f in range(2):
            ref = od.match(pairs[f][1], 78.0)
            assert len(got[f]) == len(ref)
            for k in ref.dtype.names:
                assert np.array_equal(got[f][k], ref[k]), k
    g.close()


def test_gray_cluster_chain():
    bank = synth.make_bank(400, seed=81)
    pairs = [gray_of(synth.make_scene(bank, 640, 480, seed=82 + f, n_instances=6)[0]) for f in range(3)]
    rng = np.random.default_rng(5)
    n_t, step, cthr, thr = 400, 10, 2, 75.0
    dists = 0.5 + 0.1 * (np.arange(n_t) % 6) + rng.uniform(-0.005, 0.005, n_t)
    rects = np.stack([np.zeros(n_t), np.zeros(n_t), [m["width"] for m in bank.meta["obj"]], [m["height"] for m in bank.meta["obj"]]], 1).astype(np.int32)
    od = o.OracleDetector(bank)
    det = Detector(bank, 640, 480, max_batch=3, max_candidates=1 << 18, gray=True)
    det.set_cluster_sidecar(dists, rects, step, 0.5, 0.1, cthr)
    det.upload([p[0] for p in pairs])
    det.enqueue(3, thr)
    got = det.collect_clusters(3, cap_total=1 << 18)
    for f in range(3):
        ref_m = od.match(pairs[f][1], thr)
        ref_c, _ = o.cluster_matches(ref_m, dists, rects, step, 0.5, 0.1, cthr)
        m, c, _ = got[f]
        same(m, ref_m)
        assert len(c) == len(ref_c)
        for k in ("index", "rect", "score", "member_count"):
            assert np.array_equal(c[k], ref_c[k]), (f, k)
    det.close()


def test_gray_and_bgr_contexts_reject_the_other_kind():
    W, H = 160, 160
    bank = synth.make_bank(10, modalities=("ColorGradient", "DepthNormal"), seed=41, size_range=(20.0, 36.0))
    frame, _ = synth.make_scene(bank, W, H, seed=42)
    g, b = gray_of(frame)
    gdet, bdet = Detector(bank, W, H, gray=True), Detector(bank, W, H)
    with pytest.raises(_lib.LmxError) as e:
        gdet.match(b, 70.0)                     # BGR source on a gray context
    assert e.value.status == _lib.LMX_ERR_SHAPE
    with pytest.raises(_lib.LmxError) as e:
        bdet.match(g, 70.0)                     # gray source on a BGR context: refused as before
    assert e.value.status == _lib.LMX_ERR_SHAPE
    for det, src in ((gdet, b), (bdet, g)):
        with pytest.raises(_lib.LmxError) as e:
            det.upload([src])
        assert e.value.status == _lib.LMX_ERR_SHAPE
    raw = [[rep3(g[0]), frame[1]]]
    with pytest.raises(_lib.LmxError) as e:
        gdet.upload_raw(raw, (W, H), (0, 0), blur3=True, mono=False)   # no colour-to-gray conversion
    assert e.value.status == _lib.LMX_ERR_SHAPE
    # both still work with their own kind, on the same bank and size (the context cache keys on the flags)
    same(gdet.match(g, 70.0), bdet.match(b, 70.0))
    gdet.close()
    bdet.close()


def test_gray_trainer_equals_trainer_on_replicated_renders(tmp_path):
    """lmx_bank_add_template on the gray renders meshsynth.render_view returns == on the same renders copied into B, G, R (what the
    reference's renderer hands addTemplate): ids, boxes, every template, and the YAML file byte for byte."""
    from linemod_pose_estimation_amd import meshsynth as ms
    chip, views = ms.load_mesh("memoryChip2"), ms.view_grid()
    for mods in (("ColorGradient", "DepthNormal"), ("ColorGradient",)):
        mdesc = [dict(DEFAULT_COLOR_GRADIENT) if m == "ColorGradient" else dict(DEFAULT_DEPTH_NORMAL) for m in mods]
        nb_g, nb_b = NativeBank.create([5, 8], mdesc), NativeBank.create([5, 8], mdesc)
        n_ok = 0
        for i in range(0, 2652, 221):
            R, dist = views[i]
            gray, depth, mask, _ = ms.render_view(chip, R, dist, ms.ENSENSO["fx"], ms.ENSENSO["fy"], 640, 480)
            rg = nb_g.add_template([gray, depth][:len(mods)], "obj", mask)
            rb = nb_b.add_template([rep3(gray), depth][:len(mods)], "obj", mask)
            assert rg == rb, (i, rg, rb)
            n_ok += rg[0] >= 0
        assert n_ok >= 5
        a, b = nb_g.to_bank(), nb_b.to_bank()
        assert a.num_templates("obj") == b.num_templates("obj") == n_ok
        for t in range(n_ok):
            for x, y in zip(a.get_templates("obj", t), b.get_templates("obj", t)):
                assert x[:3] == y[:3] and np.array_equal(x[3], y[3])
        pa, pb = tmp_path / "gray.yml", tmp_path / "bgr.yml"
        nb_g.save_yaml(pa)
        nb_b.save_yaml(pb)
        assert pa.read_bytes() == pb.read_bytes()


def test_gray_full_size_config0_every_frame():
    """BASELINE configs[0]: 640x480, ColorGradient only, 3000 templates; every frame of a 64-frame batch, device lanes, pipelined."""
    bank = synth.make_bank(3000, modalities=("ColorGradient",), T=(5, 8), seed=20250214)
    scenes = [synth.make_scene(bank, 640, 480, seed=4000 + f, row_pad=0)[0] for f in range(64)]
    pairs = [gray_of(s) for s in scenes]
    od = o.OracleDetector(bank)
    refs = [od.match(b, 92.0) for _, b in pairs]
    assert sum(len(r) for r in refs) > 64
    det = Detector(bank, 640, 480, max_batch=64, overlap=True, gray=True)
    det.upload([p[0] for p in pairs])
    for _ in range(det.max_outstanding):
        det.enqueue(64, 92.0)
    for _ in range(det.max_outstanding):
        outs = det.collect(64)
        for f in range(64):
            same(outs[f], refs[f])
    det.close()


def test_cv_facade_gray_and_bgr_calls_alternate(tmp_path):
    """cv::linemod::Detector::match with a CV_8UC1 ColorGradient source (the stand-in cv::Mat): gray and BGR calls alternate on one detector,
    each kind on a context of its own; all four calls give the oracle's matches and the same quantized images."""
    exe = str(tmp_path / "cv_gray_main")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "cv_standin"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cv_gray_main.cpp"), "-o", exe, "-pthread",
                           "-L", _lib.CSRC, "-llmx", "-Wl,-rpath," + _lib.CSRC, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    W, H, cols, crop = 320, 240, 432, 56
    for mods in (("ColorGradient",), ("ColorGradient", "DepthNormal")):
        bank = synth.make_bank(30, modalities=mods, seed=61, size_range=(24.0, 60.0))
        yml = tmp_path / "obj_templates.yml"
        NativeBank.from_bank(bank).save_yaml(yml)
        scene, _ = synth.make_scene(bank, cols, H, seed=62)
        g = np.ascontiguousarray(scene[0][:, :, 1])
        (tmp_path / "gray.raw").write_bytes(g.tobytes())
        args = [exe, str(yml), str(W), str(H), str(cols), str(crop), "74", str(tmp_path / "gray.raw")]
        src = [rep3(g[:, crop:crop + W])]
        if len(mods) == 2:
            (tmp_path / "depth.raw").write_bytes(np.ascontiguousarray(scene[1]).tobytes())
            args.append(str(tmp_path / "depth.raw"))
            src.append(np.ascontiguousarray(scene[1][:, crop:crop + W]))
        res = subprocess.run(args, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        ref = o.OracleDetector(bank).match(src, 74.0)
        assert len(ref) > 0
        blocks = res.stdout.split("call ")[1:]
        assert len(blocks) == 4
        heads = [b.splitlines()[0].split() for b in blocks]
        assert [h[1] for h in heads] == ["gray", "bgr", "gray", "bgr"]
        assert len({tuple(h[3:]) for h in heads}) == 1                 # same match count and the same quantized images in every call
        for b in blocks:
            got = [l.split() for l in b.splitlines()[1:]]
            assert len(got) == len(ref)
            for gl, r in zip(got, ref):
                assert (int(gl[0]), int(gl[1]), int(gl[3])) == (r["x"], r["y"], r["template_id"]) and gl[4] == "obj"
                assert np.float32(float(gl[2])) == r["similarity"]
