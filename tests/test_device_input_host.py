"""The host side of the device-input entry points without a GPU: the two symbols are part of the C ABI list, and device_images -- the pure
function that turns torch tensors / __cuda_array_interface__ objects into lmx_image descriptors -- on stand-ins built on the CPU: objects
that expose __cuda_array_interface__ over made-up addresses (nothing dereferences them) and CPU tensors for the refusals."""
import numpy as np
import pytest
import torch

from linemod_pose_estimation_amd import _lib, device_images
from linemod_pose_estimation_amd.detector import _device_stream


class Cai:
    """What a GPU array library hands out: shape, typestr, data pointer and (optionally) byte strides."""

    def __init__(self, shape, typestr, ptr, strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


class FakeCudaTensor:
    """A torch tensor's attributes as device_images reads them, over a CPU tensor's geometry: is_cuda, device.index, data_ptr, stride."""

    class Dev:
        def __init__(self, index):
            self.index = index

    def __init__(self, t, index=0):
        self.t, self.is_cuda, self.device, self.dtype, self.shape = t, True, self.Dev(index), t.dtype, t.shape

    def data_ptr(self):
        return self.t.data_ptr()

    def stride(self):
        return self.t.stride()


def test_the_new_entry_points_are_part_of_the_abi_list():
    assert "lmx_ctx_upload_device" in _lib.SYMBOLS and "lmx_depth_templates_upload_scene_device" in _lib.SYMBOLS
    header = open(_lib.CSRC + "/../../include/lmx.h").read()
    assert "lmx_status lmx_ctx_upload_device(" in header and "lmx_status lmx_depth_templates_upload_scene_device(" in header


def test_contiguous_sources_of_every_type():
    srcs = [Cai((48, 64, 3), "|u1", 0x1000), Cai((48, 64), "|u1", 0x2000), Cai((48, 64), "<u2", 0x3000), Cai((48, 64), "<i2", 0x4000), Cai((48, 64), "<f4", 0x5000)]
    imgs, keep = device_images([srcs])
    got = [(im.data, im.rows, im.cols, im.channels, im.elem_size, im.row_stride_bytes) for im in imgs]
    assert got == [(0x1000, 48, 64, 3, 1, 192), (0x2000, 48, 64, 1, 1, 64), (0x3000, 48, 64, 1, 2, 128), (0x4000, 48, 64, 1, 2, 128), (0x5000, 48, 64, 1, 4, 256)]
    assert keep == srcs
    assert _device_stream(keep, None) == 0 and _device_stream(keep, 0x77) == 0x77


def test_explicit_strides_and_frame_major_order():
    frames = [[Cai((48, 64, 3), "|u1", 0x1000 + 7, (1024, 3, 1)), Cai((48, 64), "<u2", 0x9000 + 2, (130, 2))],
              [Cai((48, 64, 3), "|u1", 0x20000, (193, 3, 1)), Cai((48, 64), "<u2", 0x30000, (128, 2))]]
    imgs, _ = device_images(frames)
    assert [(im.data, im.row_stride_bytes, im.channels, im.elem_size) for im in imgs] == [(0x1007, 1024, 3, 1), (0x9002, 130, 1, 2), (0x20000, 193, 3, 1), (0x30000, 128, 1, 2)]


def test_sliced_tensor_views_are_described_in_place():
    big = torch.zeros((3, 60, 80, 3), dtype=torch.uint8)
    view = big[1, 4:52, 8:72]                       # 48 x 64 x 3 inside a 60 x 80 frame: row stride of the parent, base inside it
    d16 = torch.zeros((60, 80), dtype=torch.int16)[10:58, 16:80]
    z = torch.zeros((50, 70), dtype=torch.float32)[1:49, 3:67]
    imgs, _ = device_images([[FakeCudaTensor(view), FakeCudaTensor(d16), FakeCudaTensor(z)]], device=0)
    c, d, f = imgs[0], imgs[1], imgs[2]
    assert (c.data, c.rows, c.cols, c.channels, c.elem_size, c.row_stride_bytes) == (big.data_ptr() + 60 * 240 + 4 * 240 + 8 * 3, 48, 64, 3, 1, 240)
    assert (d.data - d16.data_ptr(), d.rows, d.cols, d.channels, d.elem_size, d.row_stride_bytes) == (0, 48, 64, 1, 2, 160)   # int16 taken as u16
    assert (f.data, f.rows, f.cols, f.elem_size, f.row_stride_bytes) == (z.data_ptr(), 48, 64, 4, 280)
    if hasattr(torch, "uint16"):
        u = torch.zeros((48, 64), dtype=torch.uint16)
        assert device_images([[FakeCudaTensor(u)]])[0][0].elem_size == 2


def test_a_prepared_device_batch_holds_the_same_descriptors():
    from linemod_pose_estimation_amd import Detector
    frames = [[Cai((48, 64, 3), "|u1", 0x1000 * (f + 1), (200, 3, 1)), Cai((48, 64), "<u2", 0x100000 * (f + 1))] for f in range(3)]
    batch = Detector.prepare_device_batch(frames)
    imgs, _ = device_images(frames)
    assert (batch.n_frames, batch.n_sources) == (3, 2) and bytes(batch.imgs) == bytes(imgs)
    assert batch.keep == [s for fr in frames for s in fr]


def test_refusals():
    ok = torch.zeros((48, 64, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CPU tensor"):
        device_images([[ok]])
    with pytest.raises(ValueError, match="contiguous"):                       # every second pixel: inner stride 6
        device_images([[FakeCudaTensor(torch.zeros((48, 128, 3), dtype=torch.uint8)[:, ::2])]])
    with pytest.raises(ValueError, match="contiguous"):                       # one channel of a BGR frame: inner stride 3
        device_images([[FakeCudaTensor(ok[:, :, 1])]])
    with pytest.raises(ValueError, match="contiguous"):                       # a transposed depth frame
        device_images([[FakeCudaTensor(torch.zeros((64, 48), dtype=torch.int16).t())]])
    with pytest.raises(ValueError, match="contiguous"):
        device_images([[Cai((48, 64), "<u2", 0x1000, (256, 4))]])
    for bad in (torch.float64, torch.int32, torch.float16, torch.int8):
        with pytest.raises(ValueError, match="uint8, uint16 / int16 or float32"):
            device_images([[FakeCudaTensor(torch.zeros((48, 64), dtype=bad))]])
    with pytest.raises(ValueError, match="uint8, uint16 / int16 or float32"):
        device_images([[Cai((48, 64), "<f8", 0x1000)]])
    for shape, dt in (((48,), torch.uint8), ((2, 48, 64, 3), torch.uint8), ((48, 64, 4), torch.uint8), ((48, 64, 3), torch.int16), ((48, 64, 3), torch.float32)):
        with pytest.raises(ValueError, match="not shape"):
            device_images([[FakeCudaTensor(torch.zeros(shape, dtype=dt))]])
    with pytest.raises(ValueError, match="different devices"):
        device_images([[FakeCudaTensor(ok, 0), FakeCudaTensor(torch.zeros((48, 64), dtype=torch.int16), 1)]])
    with pytest.raises(ValueError, match="different devices"):
        device_images([[FakeCudaTensor(ok, 1)]], device=0)
    with pytest.raises(ValueError, match="__cuda_array_interface__"):
        device_images([[np.zeros((48, 64, 3), np.uint8)]])
    with pytest.raises(ValueError, match="row stride"):                       # rows that overlap
        device_images([[Cai((48, 64), "<u2", 0x1000, (64, 2))]])
