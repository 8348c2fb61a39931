"""The Python binding's own pieces (linemod_pose_estimation_amd/detector.py) without a device: the signatures of the public calls whose
bodies share helpers, the pure layout builders of the two pose chains, the record helper every to_host() reads its tensors with (on CPU
tensors), the binder of a chain descriptor's array fields from lists in host memory, and the offsets / class_base normalisers."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from linemod_pose_estimation_amd import MATCH_DTYPE, POSE_REFINE_DTYPE, POSE_VERIFY_DTYPE, ROUGH_POSE_DTYPE, ExportedPoses, ExportedRoughPoses, _lib, pose_chain_layout, rough_pose_layout
from linemod_pose_estimation_amd import detector as D
from linemod_pose_estimation_amd.detector import CLUSTER_DTYPE

# str(inspect.signature(f)) of every name at the commit before the binding's helpers were shared
SIGNATURES = {
    "export_layout": "(n_frames, clusters=False, caps=(65536, 4096, 65536))",
    "export_clusters_layout": "(n_frames, score=0, classes=False, caps=(65536, 4096, 65536))",
    "pose_chain_layout": "(cap_clusters)",
    "rough_pose_layout": "(cap_clusters, cap_members)",
    "ExportedMatches.__init__": "(self, n_frames, clusters, caps, stream, device)",
    "ExportedClusters.__init__": "(self, n_frames, score, classes, caps, stream, device)",
    "ExportedPoses.__init__": "(self, cap_clusters, stream, device)",
    "ExportedRoughPoses.__init__": "(self, cap_clusters, cap_members, stream, device)",
    "Detector.export_matches": "(self, n_frames, clusters=False, oldest=False, max_large_frames=0, cap_matches=65536, cap_clusters=4096, cap_members=65536, stream=None, "
                               "out=None)",
    "Detector.export_clusters": "(self, n_frames, templates=None, class_index=-1, normals=False, no_value=-inf, classes=False, class_base=None, oldest=False, "
                                "max_large_frames=0, cap_matches=65536, cap_clusters=4096, cap_members=65536, stream=None, out=None)",
    "Detector.collect_clusters": "(self, n_frames, cap_total=65536)",
    "Detector.collect_clusters_depth": "(self, n_frames, templates, class_index=-1, no_value=-inf, cap_total=65536)",
    "Detector.collect_clusters_depth_normal": "(self, n_frames, templates, class_index=-1, no_value=-inf, cap_total=65536)",
    "Detector.collect_clusters_classes": "(self, n_frames, templates=None, class_base=None, normals=False, no_value=-inf, cap_total=65536)",
    "Detector.set_cluster_sidecar": "(self, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh=2)",
    "Detector.set_cluster_sidecar_class": "(self, class_index, obj_origin_dists, rects, vote_row_col_step=1, renderer_radius_min=0.0, renderer_radius_step=1.0, "
                                          "cluster_size_thresh=2)",
    "DepthTemplates.diff": "(self, depth_frames, matches, offsets=None, class_index=-1)",
    "DepthTemplates.normal_diff": "(self, depth_frames, matches, offsets=None, class_index=-1)",
    "DepthTemplates.refine_poses": "(self, matches, depth_frames=None, offsets=None, class_index=-1, model_camera=None, scene_camera=None, max_dist_mm=10.0, "
                                   "max_iterations=20, min_pairs=16, search_radius=1, eps_rot_rad=1e-05, eps_trans_mm=0.001, rects=None)",
    "DepthTemplates.verify_poses": "(self, matches, poses, depth_frames=None, offsets=None, class_index=-1, model_camera=None, scene_camera=None, voxel_mm=4.0, "
                                   "roi_margin=8, rects=None)",
    "DepthTemplates.pose_chain": "(self, exported, keep_thresh, model_camera=None, scene_camera=None, max_dist_mm=10.0, max_iterations=20, min_pairs=16, search_radius=1, "
                                 "eps_rot_rad=1e-05, eps_trans_mm=0.001, voxel_mm=4.0, roi_margin=8, rects=None, class_index=-1, class_base=None, stream=None, out=None)",
    "DepthTemplates.rough_pose_chain": "(self, exported, model, keep_thresh, threshold_deg=10.0, scene_camera=None, model_camera=None, max_dist_mm=10.0, max_iterations=20, "
                                       "min_pairs=16, search_radius=1, eps_rot_rad=1e-05, eps_trans_mm=0.001, voxel_mm=4.0, roi_margin=8, class_index=-1, trace_min=None, "
                                       "stream=None, out=None)",
    "DepthTemplates.debug_pose_chain": "(self, header, frame_info, matches, clusters, members, keep_thresh, cap_clusters=None, fill=0, class_index=-1, class_base=None, "
                                       "model_camera=None, scene_camera=None, max_dist_mm=10.0, max_iterations=20, min_pairs=16, search_radius=1, eps_rot_rad=1e-05, "
                                       "eps_trans_mm=0.001, voxel_mm=4.0, roi_margin=8, rects=None)",
    "DepthTemplates.debug_rough_pose_chain": "(self, model, header, frame_info, matches, clusters, members, keep_thresh, threshold_deg=10.0, cap_clusters=None, fill=0, "
                                             "class_index=-1, trace_min=None, scene_camera=None, model_camera=None, max_dist_mm=10.0, max_iterations=20, min_pairs=16, "
                                             "search_radius=1, eps_rot_rad=1e-05, eps_trans_mm=0.001, voxel_mm=4.0, roi_margin=8)",
    "cluster_matches": "(matches, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh=2)",
    "cluster_matches_scored": "(matches, match_values, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh=2)",
    "cluster_matches_classes": "(matches, classes, match_values=None)",
    "debug_device_finalize_cluster": "(records, n_frames, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh=2, "
                                     "device=0, with_counts=False, large=False)",
    "debug_device_finalize_cluster_depth": "(records, n_frames, templates, depth_frames, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, "
                                           "renderer_radius_step, cluster_size_thresh=2, class_index=-1, no_value=-inf, device=0, with_counts=False, large=False)",
    "debug_device_finalize_cluster_classes": "(records, n_frames, classes, templates=None, class_base=None, depth_frames=None, normals=False, no_value=-inf, device=0, "
                                             "with_counts=False, large=False)",
    "debug_device_finalize_cluster_large": "(*args, **kw)",
    "debug_device_finalize_cluster_large_depth": "(*args, **kw)",
    "debug_device_finalize_cluster_large_classes": "(*args, **kw)",
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures_are_pinned(name):
    obj = D
    for part in name.split("."):
        obj = getattr(obj, part)
    assert str(inspect.signature(obj)) == SIGNATURES[name]


# ---- the layouts of the two pose chains ----------------------------------------------------------------------------------------------------
RECORD_BYTES = {"poses": (136, POSE_REFINE_DTYPE), "checks": (48, POSE_VERIFY_DTYPE), "rough": (152, ROUGH_POSE_DTYPE)}


def check_entries(lay, want):
    """want: name -> (shape, dtype, align, cap), in the layout's order"""
    assert list(lay) == list(want)
    for k, (shape, dtype, align, cap) in want.items():
        assert list(lay[k]) == ["shape", "dtype", "nbytes", "align", "cap"], k
        assert (lay[k]["shape"], lay[k]["dtype"], lay[k]["align"], lay[k]["cap"]) == (shape, dtype, align, cap), k
        assert lay[k]["nbytes"] == int(np.prod(shape)) * np.dtype(dtype).itemsize and type(lay[k]["nbytes"]) is int, k
        if k in RECORD_BYTES:
            literal, dt = RECORD_BYTES[k]
            assert dt.itemsize == literal and shape[1] * 8 == literal and lay[k]["nbytes"] == cap * literal, k


@pytest.mark.parametrize("cap", [1, 5, 1 << 20])
def test_pose_chain_layout(cap):
    check_entries(pose_chain_layout(cap), {"chain_header": ((8,), "int32", 4, 8), "leaders": ((cap,), "int32", 4, cap), "poses": ((cap, 17), "int64", 8, cap),
                                           "checks": ((cap, 6), "int64", 8, cap), "keep": ((cap,), "uint8", 1, cap)})
    assert tuple(pose_chain_layout(cap)) == ExportedPoses.NAMES


@pytest.mark.parametrize("cap", [1, 5, 1 << 20])
@pytest.mark.parametrize("cap_members", [0, 1, 7])
def test_rough_pose_layout(cap, cap_members):
    n_mem = max(cap_members, 1)
    lay = rough_pose_layout(cap, cap_members)
    check_entries(lay, {"chain_header": ((8,), "int32", 4, 8), "poses": ((cap, 17), "int64", 8, cap), "checks": ((cap, 6), "int64", 8, cap),
                        "keep": ((cap,), "uint8", 1, cap), "rough": ((cap, 19), "int64", 8, cap), "member_group": ((n_mem,), "int32", 4, n_mem)})
    assert sorted(lay) == sorted(ExportedRoughPoses.NAMES)


def test_rough_pose_layout_keeps_one_member_element():
    assert rough_pose_layout(5, 0)["member_group"] == {"shape": (1,), "dtype": "int32", "nbytes": 4, "align": 4, "cap": 1}


@pytest.mark.parametrize("cap", [0, (1 << 20) + 1])
def test_chain_layouts_refuse_a_capacity_out_of_range(cap):
    with pytest.raises(ValueError, match=r"cap_clusters must be 1 \.\. 2\^20"):
        pose_chain_layout(cap)
    with pytest.raises(ValueError, match=r"cap_clusters must be 1 \.\. 2\^20"):
        rough_pose_layout(cap, 4)


# ---- the record helper ------------------------------------------------------------------------------------------------------------------------
def known_records(dtype, n):
    """n records of `dtype` made of known bytes, pads included; no two records are equal"""
    raw = (np.arange(n * dtype.itemsize, dtype=np.uint32) * 37 + 11).astype(np.uint8)
    return raw.view(dtype).reshape(-1)


@pytest.mark.parametrize("torch_dtype, row, dtype", [(torch.int64, 17, POSE_REFINE_DTYPE), (torch.uint8, 48, CLUSTER_DTYPE), (torch.int32, 5, MATCH_DTYPE)])
def test_records_come_back_byte_for_byte(torch_dtype, row, dtype):
    rows = 4 if dtype is POSE_REFINE_DTYPE else 3
    want = known_records(dtype, rows)
    word = {torch.int64: np.int64, torch.uint8: np.uint8, torch.int32: np.int32}[torch_dtype]
    t = torch.from_numpy(want.view(word).reshape(rows, row).copy())
    assert t.dtype == torch_dtype and tuple(t.shape) == (rows, row) and want.itemsize == row * t.element_size()
    for n in (0, rows - 1, rows, min(9, rows)):                 # the last: a count beyond the capacity, clamped as to_host() clamps it
        got = D._records(t, n, dtype)
        assert got.dtype == dtype and got.shape == (n,) and got.flags["C_CONTIGUOUS"]
        assert got.tobytes() == want[:n].tobytes()
    assert D._records(t, 9, dtype).tobytes() == want.tobytes()  # unclamped, the slice ends with the tensor
    assert t.numpy().tobytes() == want.tobytes()                # and the tensor is as it was


def test_records_of_a_one_dimensional_tensor():
    t = torch.arange(7, dtype=torch.int32)
    assert D._records(t, 3, np.int32).tolist() == [0, 1, 2] and D._records(t, 0, np.int32).shape == (0,)


# ---- a chain descriptor's array fields from lists in host memory ---------------------------------------------------------------------------
FILL = 0xA5
INPUTS = ("header", "frame_info", "matches", "clusters", "members")


def host_lists():
    header = np.zeros(16, np.int32)
    header[:5] = (2, -1, 4, 3, 5)                       # a negative word: the flags with every bit set
    frame_info = [0, 3, 0, 2, 0, 4, 0, 3, 3, 1, 2, 1, 4, 1, 0, 1]            # two frames, flat
    return header, frame_info, known_records(MATCH_DTYPE, 4), known_records(CLUSTER_DTYPE, 3), [0, 1, 2, 0, 3]


@pytest.mark.parametrize("desc, names", [(_lib.PoseChainDesc, ExportedPoses.NAMES), (_lib.RoughChainDesc, ExportedRoughPoses.NAMES)])
@pytest.mark.parametrize("cap_clusters", [None, 2])
def test_host_lists_bind_to_a_descriptor(desc, names, cap_clusters):
    d = desc()
    lists = D._chain_inputs_host(d, host_lists(), cap_clusters)
    header, frame_info, matches, clusters, members = lists
    assert header.dtype == np.uint32 and header.shape == (16,) and header[1] == 0xFFFFFFFF and header[0] == 2
    assert frame_info.dtype == np.int32 and frame_info.shape == (2, 8) and frame_info[1].tolist() == [3, 1, 2, 1, 4, 1, 0, 1]
    assert matches.dtype == MATCH_DTYPE and clusters.dtype == CLUSTER_DTYPE and members.dtype == np.int32 and members.tolist() == [0, 1, 2, 0, 3]
    assert matches.tobytes() == host_lists()[2].tobytes() and clusters.tobytes() == host_lists()[3].tobytes()
    assert all(a.flags["C_CONTIGUOUS"] for a in lists)
    assert [getattr(d, k) for k in INPUTS] == [a.ctypes.data for a in lists]
    assert (d.cap_matches, d.cap_clusters, d.cap_members) == (4, 3 if cap_clusters is None else 2, 5)

    out = D._chain_outputs_host(names, len(clusters), len(members), FILL)
    assert tuple(out) == names
    D._chain_outputs(d, names, {k: a.ctypes.data for k, a in out.items()})
    assert [getattr(d, k) for k in names] == [out[k].ctypes.data for k in names]
    assert out["chain_header"].dtype == np.uint32 and out["chain_header"].shape == (8,) and not out["chain_header"].any()
    for k in names[1:]:
        assert len(out[k]) == (5 if k == "member_group" else 3), k
        assert (out[k].view(np.uint8) == FILL).all(), k
    assert out["poses"].dtype == POSE_REFINE_DTYPE and out["checks"].dtype == POSE_VERIFY_DTYPE and out["keep"].dtype == np.uint8
    assert [getattr(d, k) for k in INPUTS] == [a.ctypes.data for a in lists]       # the outputs left the inputs alone


def test_host_lists_refuse_a_capacity_beyond_the_clusters():
    with pytest.raises(ValueError, match=r"cap_clusters exceeds len\(clusters\)"):
        D._chain_inputs_host(_lib.PoseChainDesc(), host_lists(), 4)


def test_member_group_keeps_one_element_without_members():
    out = D._chain_outputs_host(ExportedRoughPoses.NAMES, 0, 0, FILL)
    assert len(out["member_group"]) == 1 and len(out["rough"]) == 0 and out["rough"].dtype == ROUGH_POSE_DTYPE


# ---- offsets and class_base -------------------------------------------------------------------------------------------------------------------
def test_frame_offsets():
    offs = D._frame_offsets(None, 1, 7)
    assert isinstance(offs, C.c_size_t * 2) and list(offs) == [0, 7]
    assert list(D._frame_offsets(np.asarray([0, 2, 2, 7]), 3, 7)) == [0, 2, 2, 7]
    with pytest.raises(ValueError, match="offsets are needed with more than one frame"):
        D._frame_offsets(None, 2, 7)
    for bad, n_frames in (([0, 7], 2), ([0, 3, 6], 2), ([0, 7, 7], 1)):
        with pytest.raises(ValueError, match=r"offsets must have one entry per frame plus one and end at len\(matches\)"):
            D._frame_offsets(bad, n_frames, 7)


def test_class_base():
    base = D._class_base([[0, 2], [5, 9]])
    assert base.dtype == np.int32 and base.tolist() == [0, 2, 5, 9] and base.flags["C_CONTIGUOUS"]
    for bad in ([], [3]):
        with pytest.raises(ValueError, match="class_base must hold one entry per class plus one"):
            D._class_base(bad)
