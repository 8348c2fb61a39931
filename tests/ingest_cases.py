"""Shared by tests/test_ingest_kernel_host.py and tests/test_gpu_device_input.py: the launches the ingest kernel of lmx_ctx_upload_device
(csrc/lmx_ingest.hpp) is checked on -- a 184x176 raw frame cropped to 160x160 at crops that touch every edge of the source and at an odd
offset, a 187x176 one whose rows are no multiple of 4 bytes, with and without the 3x3 blur, BGR and MONO8 sources into BGR and gray
frames, u16 depth and float depth tiled with the values at which the metre -> millimetre conversion can go wrong -- and the ways a source
image may lie in memory: three pitches (packed, packed + one element, 1024 bytes) and a base 0 to 16 bytes off a 64-byte boundary."""
import struct

import numpy as np

import np_restatement as npr

W = H = 160
RAW, RAW_ODD = (184, 176), (187, 176)          # (SW, SH)
CROPS = [(0, 0), (24, 16), (24, 0), (0, 16), (11, 7)]
CROPS_ODD = [(27, 16)]
DEPTH_EXTRA_CROPS = [(13, 3), (6, 1)]           # float windows that start 4 and 8 bytes into a 16-byte granule
KINDS = ("bgr", "mono_on_bgr_context", "mono_on_gray_context")
FILL = 0xA5                                     # what lies between the rows and around the image


def placements(row_bytes, es, salt):
    """-> two lists of three (pitch, base offset) each, one per frame of a call.  Offsets are multiples of the element size `es`."""
    off = lambda k: es * (1 + (salt + k) % (15 // es))   # noqa: E731
    return ([(row_bytes, 0), (row_bytes + es, off(0)), (1024, 0)],
            [(1024, off(1)), (1024, 16), (row_bytes, off(2))])


def place(image, pitch, offset):
    """A copy of `image` (rows of contiguous elements) with row pitch `pitch` bytes whose first byte lies `offset` bytes behind a 64-byte
    boundary -> (the buffer that keeps it alive, its address).  At least 16 bytes follow the last row."""
    image = np.ascontiguousarray(image)
    rows = image.reshape(image.shape[0], -1).view(np.uint8)
    assert pitch >= rows.shape[1]
    buf = np.full(64 + offset + rows.shape[0] * pitch + 16, FILL, np.uint8)
    base = (-buf.ctypes.data) % 64 + offset
    np.lib.stride_tricks.as_strided(buf[base:], shape=rows.shape, strides=(pitch, 1))[...] = rows
    return buf, buf.ctypes.data + base


def raw_frames(size, seed):
    """-> three BGR frames, three float-metre depth frames (every special value in every crop) and three u16 depth frames of `size`."""
    SW, SH = size
    bgr, z, table, n_even, n_odd = npr.pre_special_frames(SW, SH, seed)
    assert n_even >= 32 and n_odd >= 32
    rng = np.random.default_rng(seed + 1)
    d16 = [rng.integers(0, 65536, (SH, SW), dtype=np.uint16) for _ in range(3)]
    return ([bgr, np.ascontiguousarray(bgr[::-1, ::-1]), np.ascontiguousarray(bgr[::-1])],
            [z, np.ascontiguousarray(z[::-1, ::-1]), np.ascontiguousarray(z[::-1])], d16)


def color_sources(kind, bgr_frames):
    """The colour sources of `kind` from three BGR frames: the frames, or one channel of each."""
    return bgr_frames if kind == "bgr" else [np.ascontiguousarray(b[:, :, 1 + f % 2]) for f, b in enumerate(bgr_frames)]


def expected_color(o, kind, source, crop, blur):
    ref = o.pre_color(source, crop, (W, H), blur)
    return np.ascontiguousarray(ref[..., 0]) if kind == "mono_on_gray_context" else ref


def launches(o):
    """Every launch: dicts with color, sc, dc, blur, depth_float, size (SW, SH), crop, name, frames [three source arrays] and expected
    [three arrays], the latter from the oracle `o` (pre_color / pre_depth), computed once per (source, crop, blur)."""
    out = []
    for size, crops in ((RAW, CROPS), (RAW_ODD, CROPS_ODD)):
        bgr, zs, d16 = raw_frames(size, 71 + size[0])
        for kind in KINDS:
            src = color_sources(kind, bgr)
            sc, dc = (3, 3) if kind == "bgr" else (1, 1 if kind == "mono_on_gray_context" else 3)
            for crop in crops:
                for blur in (True, False):
                    out.append({"color": 1, "sc": sc, "dc": dc, "blur": int(blur), "depth_float": 0, "size": size, "crop": crop, "frames": src,
                                "name": "%s %dx%d crop %s blur %d" % (kind, size[0], size[1], crop, blur),
                                "expected": [expected_color(o, kind, s, crop, blur) for s in src]})
        for crop in crops + (DEPTH_EXTRA_CROPS if size == RAW else []):
            (cx, cy) = crop
            out.append({"color": 0, "sc": 1, "dc": 1, "blur": 0, "depth_float": 1, "size": size, "crop": crop, "frames": zs,
                        "name": "float depth %dx%d crop %s" % (size[0], size[1], crop), "expected": [o.pre_depth(z, crop, (W, H)) for z in zs]})
            out.append({"color": 0, "sc": 1, "dc": 1, "blur": 0, "depth_float": 0, "size": size, "crop": crop, "frames": d16,
                        "name": "u16 depth %dx%d crop %s" % (size[0], size[1], crop), "expected": [np.ascontiguousarray(d[cy:cy + H, cx:cx + W]) for d in d16]})
    # frame-sized sources: taken as they are (the blur sees both borders in one window row), and the plain pitched copy of pre == NULL
    bgr, zs, d16 = raw_frames((W, H), 90)
    for kind in KINDS:
        src = color_sources(kind, bgr)
        sc, dc = (3, 3) if kind == "bgr" else (1, 1 if kind == "mono_on_gray_context" else 3)
        for blur in (True, False):
            out.append({"color": 1, "sc": sc, "dc": dc, "blur": int(blur), "depth_float": 0, "size": (W, H), "crop": (0, 0), "frames": src,
                        "name": "%s frame-sized blur %d" % (kind, blur), "expected": [expected_color(o, kind, s, (0, 0), blur) for s in src]})
    out.append({"color": 0, "sc": 1, "dc": 1, "blur": 0, "depth_float": 0, "size": (W, H), "crop": (0, 0), "frames": d16, "name": "u16 depth frame-sized",
                "expected": list(d16)})
    return out


def element_size(case):
    return 1 if case["color"] else (4 if case["depth_float"] else 2)


def source_row_bytes(case):
    return case["size"][0] * (case["sc"] if case["color"] else element_size(case))


def write_cases(path, cases):
    """The file tests/cpp/ingest_main.cpp reads: every case once per placement list -> the number of launches written."""
    n = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<i", 2 * len(cases)))
        for ci, c in enumerate(cases):
            (SW, SH), (cx, cy) = c["size"], c["crop"]
            for lay in placements(source_row_bytes(c), element_size(c), ci):
                f.write(struct.pack("<12i", c["color"], c["sc"], c["dc"], c["blur"], c["depth_float"], SH, SW, H, W, cx, cy, len(lay)))
                for (pitch, offset), src, exp in zip(lay, c["frames"], c["expected"]):
                    f.write(struct.pack("<2i", pitch, offset))
                    f.write(np.ascontiguousarray(src).tobytes())
                    f.write(np.ascontiguousarray(exp).tobytes())
                n += 1
    return n
