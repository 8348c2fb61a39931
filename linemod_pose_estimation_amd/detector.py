"""Python host-side mirror of the reference's operator surface for the matching path.

`Detector` keeps the names and argument meaning of cv::linemod::Detector as the reference uses it:
  readLinemod(filename)                    /root/reference/src/rgbdDetector.cpp:1668-1680
  detector.match(sources, threshold, ...)  /root/reference/src/rgbdDetector.cpp:31-34
  detector.classIds(), getTemplates(), numTemplates(), getT(), pyramidLevels()
Everything computes through the C ABI of liblmx.so (include/lmx.h) on a gfx950 device; there is no CPU path here.
"""
import copy
import ctypes as C
from collections.abc import Mapping

import numpy as np

from . import _lib
from .bank import TemplateBank

MATCH_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("similarity", "<f4"), ("template_id", "<i4"), ("class_index", "<i4")])
RAW_MATCH_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("similarity", "<f4"), ("template_id", "<i4"),
                            ("class_index", "<i4"), ("frame", "<i4"), ("order_key", "<u8")])
CLUSTER_DTYPE = np.dtype([("index", "<i4", (3,)), ("rect", "<i4", (4,)), ("score", "<f8"), ("member_begin", "<i4"), ("member_count", "<i4")],
                         align=True)
DEPTH_DIFF_DTYPE = np.dtype([("sum_abs_mm", "<i8"), ("n_valid", "<i4"), ("n_template", "<i4")])
NORMAL_DIFF_DTYPE = np.dtype([("sum_angle_urad", "<i8"), ("n_normal", "<i4"), ("reserved", "<i4")])
# the host lists of the collect_clusters* calls and of the debug_device_finalize_cluster* hooks, by the short names their helpers take
_LIST_DTYPES = {"m": MATCH_DTYPE, "d": DEPTH_DIFF_DTYPE, "nd": NORMAL_DIFF_DTYPE, "cl": CLUSTER_DTYPE, "cc": np.int32, "mem": np.int32}


def _images(frames):
    """frames: list (per frame) of list (per modality) of numpy arrays -> ctypes Image array (+ keep-alive)."""
    flat = [s for fr in frames for s in fr]
    arr = (_lib.Image * len(flat))()
    for i, s in enumerate(flat):
        if s.dtype == np.uint8 and s.ndim == 3:
            ch, es = s.shape[2], 1
            ok = s.strides[2] == 1 and s.strides[1] == ch
        elif s.dtype == np.uint8 and s.ndim == 2:        # MONO8 (upload_raw with mono=True)
            ch, es = 1, 1
            ok = s.strides[1] == 1
        elif s.dtype == np.uint16 and s.ndim == 2:
            ch, es = 1, 2
            ok = s.strides[1] == 2
        elif s.dtype == np.float32 and s.ndim == 2:      # depth in metres (upload_raw with depth_float_m=True)
            ch, es = 1, 4
            ok = s.strides[1] == 4
        else:
            raise TypeError("sources must be uint8 HxWx3 / HxW (colour) or uint16 / float32 HxW (depth)")
        if not ok:
            raise TypeError("source pixels must be contiguous within a row (row stride may be larger)")
        arr[i] = _lib.Image(s.ctypes.data, s.shape[0], s.shape[1], ch, es, s.strides[0])
    return arr, flat


_DEVICE_DTYPES = {"uint8": 1, "uint16": 2, "int16": 2, "float32": 4}      # int16 is taken as its bit pattern (torch before 2.3 has no uint16)
_CAI_TYPES = {"|u1": 1, "<u2": 2, "<i2": 2, "<f4": 4}


def _device_view(s):
    """One source in device memory -> (address, shape, strides in bytes, element size, device index or None, is a torch tensor).
    torch tensors are recognised by their attributes (torch is not imported here); anything else needs __cuda_array_interface__."""
    if hasattr(s, "data_ptr") and hasattr(s, "is_cuda"):
        if not s.is_cuda:
            raise ValueError("upload_device takes tensors in device memory: a CPU tensor goes through upload()")
        es = _DEVICE_DTYPES.get(str(s.dtype).replace("torch.", ""))
        if es is None:
            raise ValueError("device sources are uint8, uint16 / int16 or float32, not %s" % (s.dtype,))
        return int(s.data_ptr()), tuple(int(v) for v in s.shape), tuple(int(v) * es for v in s.stride()), es, s.device.index, True
    try:
        cai = s.__cuda_array_interface__
    except AttributeError:
        raise ValueError("a device source is a torch tensor on the GPU or an object with __cuda_array_interface__, not %s" % type(s).__name__)
    es = _CAI_TYPES.get(cai["typestr"])
    if es is None:
        raise ValueError("device sources are uint8, uint16 / int16 or float32, not %r" % (cai["typestr"],))
    shape = tuple(int(v) for v in cai["shape"])
    strides = cai.get("strides")
    if strides is None:     # C-contiguous
        strides, run = [], es
        for n in reversed(shape):
            strides.insert(0, run)
            run *= n
    return int(cai["data"][0]), shape, tuple(int(v) for v in strides), es, None, False


def device_images(frames, device=None):
    """frames: list (per frame) of list (per modality) of sources in device memory -- torch tensors on one GPU (on `device` when given)
    or objects with __cuda_array_interface__: uint8 HxWx3 / HxW, uint16 or int16 HxW, float32 HxW.  Views and slices are described in
    place: the row stride is the source's own, the elements of a row must be contiguous.  -> (ctypes lmx_image array, keep-alive).
    ValueError: a CPU tensor, a non-unit inner stride, a wrong dtype or rank, tensors on different devices."""
    flat = [s for fr in frames for s in fr]
    arr = (_lib.Image * max(1, len(flat)))()
    seen = device
    for i, s in enumerate(flat):
        ptr, shape, strides, es, dev, _ = _device_view(s)
        if len(shape) == 3 and es == 1 and shape[2] == 3:
            ch, ok = 3, strides[2] == 1 and strides[1] == 3
        elif len(shape) == 2:
            ch, ok = 1, strides[1] == es
        else:
            raise ValueError("device sources are uint8 HxWx3 / HxW (colour) or uint16 / int16 / float32 HxW (depth), not shape %s of %d-byte elements" % (shape, es))
        if not ok:
            raise ValueError("the elements of a row must be contiguous (the row stride may be larger): strides %s bytes" % (strides,))
        if strides[0] < shape[1] * ch * es:
            raise ValueError("row stride %d bytes is below the row's %d bytes" % (strides[0], shape[1] * ch * es))
        if dev is not None:
            if seen is not None and dev != seen:
                raise ValueError("device sources on different devices (%s and %s)" % (seen, dev))
            seen = dev
        arr[i] = _lib.Image(ptr, shape[0], shape[1], ch, es, strides[0])
    return arr, flat


def _device_stream(flat, stream):
    """stream=None: the current torch stream of the tensors' device, or the null stream for other sources."""
    if stream is not None:
        return int(getattr(stream, "cuda_stream", stream))
    if flat and hasattr(flat[0], "is_cuda"):
        import torch
        return int(torch.cuda.current_stream(flat[0].device).cuda_stream)
    return 0


EXPORT_HEADER_WORDS, EXPORT_INFO_WORDS = 16, 8
EXPORT_INFO_FIELDS = ("match_begin", "match_count", "cluster_begin", "cluster_count", "member_begin", "member_count", "status", "raw_records")
# frame_info's status and header[1]'s flags (include/lmx.h, lmx_ctx_export_matches_on)
EXPORT_DELIVERED, EXPORT_UNFINISHED, EXPORT_RANGE, EXPORT_MATCHES_NO_FIT, EXPORT_CLUSTERS_NO_FIT, EXPORT_OVERFLOW = 0, 1, 2, 4, 8, 16
EXPORT_FLAG_OVERFLOW, EXPORT_FLAG_UNFINISHED, EXPORT_FLAG_NO_FIT = 1, 2, 4


def _entry(shape, dtype, align, cap):
    """One array of a layout, as export_layout describes it."""
    return {"shape": shape, "dtype": dtype, "nbytes": int(np.prod(shape)) * np.dtype(dtype).itemsize, "align": align, "cap": cap}


def _records(t, n, dtype):
    """The first n records of the tensor t (on the GPU or the CPU; a record is a row, or an element of a 1-D tensor) -> numpy array [n]
    of `dtype`, whose itemsize is the record's."""
    return np.ascontiguousarray(t[:n].cpu().numpy()).view(dtype).reshape(-1)


def _torch_stream(stream, default, device):
    """The stream argument of the export and chain calls -> a torch stream: a torch stream as it is, a raw hipStream_t wrapped; None:
    `default`, or without one the current torch stream of `device`."""
    import torch
    if stream is None:
        return default if default is not None else torch.cuda.current_stream(device)
    return stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=device)


class _Exported:
    """What the Exported* classes share: tensors allocated from a layout on a stream (`_backing`, name -> tensor), the named views of them
    that a subclass's _views() binds, and the copy."""

    def _allocate(self, lay, stream, device):
        import torch
        self.stream = stream
        with torch.cuda.stream(stream):     # the caching allocator hands out memory that is free on this stream
            self._backing = {k: torch.empty(v["shape"], dtype=getattr(torch, v["dtype"]), device="cuda:%d" % device) for k, v in lay.items()}
        self._views()

    @property
    def similarity(self):
        import torch
        return self.matches[:, 2].view(torch.float32)

    def _delivered(self):
        """Synchronises `stream` -> (an export's frame_info on the host, how many matches, clusters and members its tensors hold)."""
        self.stream.synchronize()
        return self.frame_info.cpu().numpy(), tuple(min(int(v), cap) for v, cap in zip(self.header[2:5].cpu().numpy(), self.caps))

    def _live(self):
        """Synchronises `stream` -> (a chain's chain_header as int64 [8], how many of its slots the tensors hold)."""
        self.stream.synchronize()
        hdr = self.chain_header.cpu().numpy().view(np.uint32).astype(np.int64)
        return hdr, min(int(hdr[0]), self.cap)

    def clone(self):
        """A copy made on `stream` (behind the call that wrote these tensors, in front of whatever writes them next): what a pipeline
        keeps of a result whose buffers the next call with out=... reuses.  Nothing waits on the host."""
        import torch
        out = copy.copy(self)       # the plain attributes; the tensors are replaced below
        with torch.cuda.stream(self.stream):
            out._backing = {k: v.clone() for k, v in self._backing.items()}
        out._views()
        return out

    @classmethod
    def _fresh_or(cls, out, made_for, caps, stream, device):
        """What an export writes and the capacities it may use.  out None: a fresh object for `made_for`, the constructor's arguments in
        front of caps, with its own capacities; else `out`, which must have been made for the same, with the smaller of `caps` and its
        own, and `stream` from now on."""
        if out is None:
            out = cls(*made_for, caps, stream, device)
            return out, out.caps
        if out._made_for() != made_for:
            raise ValueError(cls.MADE_FOR % out._made_for())
        out.stream = stream
        return out, tuple(min(int(a), b) for a, b in zip(caps, out.caps))


def export_layout(n_frames, clusters=False, caps=(1 << 16, 4096, 1 << 16)):
    """The device arrays lmx_ctx_export_matches_on fills, as Detector.export_matches allocates them: name -> {"shape", "dtype" (a numpy
    dtype name, the torch dtype of the same name), "nbytes", "align" (of the address, the C ABI's rule), "cap" (elements the call may
    write)}.  caps = (cap_matches, cap_clusters, cap_members); the cluster and member arrays exist with clusters=True only.  A capacity of 0
    is allowed: the array keeps one element so that it has an address, and nothing is written to it.
    ValueError: n_frames < 1, a negative capacity, or a capacity whose offsets would not fit frame_info's int32."""
    caps = tuple(int(v) for v in caps)
    if n_frames < 1:
        raise ValueError("n_frames must be at least 1")
    if len(caps) != 3 or min(caps) < 0 or max(caps) >= 1 << 31:
        raise ValueError("caps = (cap_matches, cap_clusters, cap_members), each 0 .. 2^31 - 1")
    out = {"header": _entry((EXPORT_HEADER_WORDS,), "int32", 4, EXPORT_HEADER_WORDS),
           "frame_info": _entry((int(n_frames), EXPORT_INFO_WORDS), "int32", 4, int(n_frames)),
           "matches": _entry((max(caps[0], 1), MATCH_DTYPE.itemsize // 4), "int32", 4, caps[0])}
    if clusters:
        out["clusters"] = _entry((max(caps[1], 1), CLUSTER_DTYPE.itemsize), "uint8", 8, caps[1])
        out["members"] = _entry((max(caps[2], 1),), "int32", 4, caps[2])
    return out


class ExportedMatches(_Exported):
    """What Detector.export_matches leaves on the GPU (lmx_ctx_export_matches_on): torch tensors on the context's device, valid for work
    queued on `stream` after the call --
      header      int32 [16]      [0] n_frames, [1] flags, [2] matches, [3] clusters, [4] members (true totals), [5] candidates, [6] raw records
      frame_info  int32 [F, 8]    EXPORT_INFO_FIELDS per frame; status 0 = delivered
      matches     int32 [cap, 5]  x, y, the similarity's bits, template_id, class_index; `similarity` is column 2 as float32
      clusters    uint8 [cap, 48] lmx_cluster_t records (CLUSTER_DTYPE); members int32 [cap]   (None without clusters=True)
    Any other stream, or the host, synchronises with `stream` first; to_host() does."""

    MADE_FOR = "out was made for %d frames, clusters=%s"

    def __init__(self, n_frames, clusters, caps, stream, device):
        self.n_frames, self.with_clusters = n_frames, bool(clusters)
        lay = export_layout(n_frames, clusters, caps)
        self.caps = tuple(lay[k]["cap"] if k in lay else 0 for k in ("matches", "clusters", "members"))
        self._allocate(lay, stream, device)

    def _made_for(self):
        return self.n_frames, self.with_clusters

    def _views(self):
        t, caps = self._backing, self.caps
        self.header, self.frame_info, self.matches = t["header"], t["frame_info"], t["matches"][:caps[0]]
        self.clusters = t["clusters"][:caps[1]] if self.with_clusters else None
        self.members = t["members"][:caps[2]] if self.with_clusters else None

    def to_host(self):
        """Synchronises `stream` -> list per frame of (matches, clusters, members) in collect_clusters' dtypes (MATCH_DTYPE, CLUSTER_DTYPE
        whose member_begin indexes `members`, the batch's flat int32 member array; both empty without clusters=True), or None for a frame
        whose status is not 0 (not finished, or an array of its did not fit)."""
        info, (n_m, n_c, n_mem) = self._delivered()
        m = _records(self.matches, n_m, MATCH_DTYPE)
        if self.with_clusters:
            cl, mem = _records(self.clusters, n_c, CLUSTER_DTYPE), _records(self.members, n_mem, np.int32)
        else:
            cl, mem = np.zeros(0, CLUSTER_DTYPE), np.zeros(0, np.int32)
        out = []
        for f in range(self.n_frames):
            mb, mc, cb, cc, _, _, status, _ = (int(v) for v in info[f])
            out.append((m[mb:mb + mc].copy(), cl[cb:cb + cc].copy(), mem) if status == EXPORT_DELIVERED else None)
        return out


def export_clusters_layout(n_frames, score=0, classes=False, caps=(1 << 16, 4096, 1 << 16)):
    """export_layout(clusters=True) plus the arrays lmx_ctx_export_clusters_on adds, as Detector.export_clusters allocates them: "diffs"
    (score >= 1) and "ndiffs" (score == 2), 16-byte records parallel to "matches" with its capacity, as int64 [cap, 2] (8-byte aligned);
    "cluster_class" (classes), int32 parallel to "clusters"."""
    if score not in (0, 1, 2):
        raise ValueError("score is 0 (mean similarity), 1 (depth) or 2 (depth + normal)")
    out = export_layout(n_frames, True, caps)
    cap_m, cap_c = out["matches"]["cap"], out["clusters"]["cap"]
    if score >= 1:
        out["diffs"] = _entry((max(cap_m, 1), DEPTH_DIFF_DTYPE.itemsize // 8), "int64", 8, cap_m)
    if score == 2:
        out["ndiffs"] = _entry((max(cap_m, 1), NORMAL_DIFF_DTYPE.itemsize // 8), "int64", 8, cap_m)
    if classes:
        out["cluster_class"] = _entry((max(cap_c, 1),), "int32", 4, cap_c)
    return out


class ExportedClusters(_Exported):
    """What Detector.export_clusters leaves on the GPU (lmx_ctx_export_clusters_on): ExportedMatches' tensors with clusters, and next to
    them, on the same device and valid for work queued on `stream` after the call --
      diffs          int64 [cap, 2]  lmx_depth_diff_t records (DEPTH_DIFF_DTYPE) parallel to matches            (None with score 0)
      ndiffs         int64 [cap, 2]  lmx_normal_diff_t records (NORMAL_DIFF_DTYPE) parallel to matches          (None unless score 2)
      cluster_class  int32 [cap]     the class of each cluster, parallel to clusters                           (None without classes)
    A frame's range of diffs / ndiffs is written iff its matches are, of cluster_class iff its clusters are."""

    MADE_FOR = "out was made for %d frames, score %d, classes=%s"

    def __init__(self, n_frames, score, classes, caps, stream, device):
        self.n_frames, self.score, self.with_classes = n_frames, int(score), bool(classes)
        lay = export_clusters_layout(n_frames, score, classes, caps)
        self.caps = tuple(lay[k]["cap"] for k in ("matches", "clusters", "members"))
        self._allocate(lay, stream, device)

    def _made_for(self):
        return self.n_frames, self.score, self.with_classes

    def _views(self):
        t, caps = self._backing, self.caps
        self.header, self.frame_info = t["header"], t["frame_info"]
        self.matches, self.clusters, self.members = t["matches"][:caps[0]], t["clusters"][:caps[1]], t["members"][:caps[2]]
        self.diffs = t["diffs"][:caps[0]] if "diffs" in t else None
        self.ndiffs = t["ndiffs"][:caps[0]] if "ndiffs" in t else None
        self.cluster_class = t["cluster_class"][:caps[1]] if "cluster_class" in t else None

    def to_host(self):
        """Synchronises `stream` -> list per frame of (matches, diffs, ndiffs, clusters, cluster_class, members) in
        collect_clusters_classes' shape and dtypes (diffs / ndiffs / cluster_class None where the call has none; CLUSTER_DTYPE's
        member_begin indexes `members`, the batch's flat member array), or None for a frame whose status is not 0."""
        info, (n_m, n_c, n_mem) = self._delivered()
        m = _records(self.matches, n_m, MATCH_DTYPE)
        d = _records(self.diffs, n_m, DEPTH_DIFF_DTYPE) if self.diffs is not None else None
        nd = _records(self.ndiffs, n_m, NORMAL_DIFF_DTYPE) if self.ndiffs is not None else None
        cl = _records(self.clusters, n_c, CLUSTER_DTYPE)
        cc = _records(self.cluster_class, n_c, np.int32) if self.cluster_class is not None else None
        mem = _records(self.members, n_mem, np.int32)
        out = []
        for f in range(self.n_frames):
            mb, mc, cb, ncl, _, _, status, _ = (int(v) for v in info[f])
            if status != EXPORT_DELIVERED:
                out.append(None)
                continue
            out.append((m[mb:mb + mc].copy(), d[mb:mb + mc].copy() if d is not None else None, nd[mb:mb + mc].copy() if nd is not None else None,
                        cl[cb:cb + ncl].copy(), cc[cb:cb + ncl].copy() if cc is not None else None, mem))
        return out


POSE_CHAIN_HEADER_WORDS = 8
POSE_CHAIN_FLAG_CUT, POSE_CHAIN_FLAG_BOUNDS, POSE_CHAIN_FLAG_POSE = 1, 2, 4      # chain_header[1] (include/lmx.h, lmx_pose_chain_on)


def pose_chain_layout(cap_clusters):
    """The device arrays lmx_pose_chain_on fills, as DepthTemplates.pose_chain allocates them, parallel to an export's clusters: name ->
    {"shape", "dtype", "nbytes", "align", "cap"} as export_layout.  ValueError: cap_clusters outside 1 .. 2^20."""
    cap = int(cap_clusters)
    if cap < 1 or cap > 1 << 20:
        raise ValueError("cap_clusters must be 1 .. 2^20")
    return {"chain_header": _entry((POSE_CHAIN_HEADER_WORDS,), "int32", 4, POSE_CHAIN_HEADER_WORDS),
            "leaders": _entry((cap,), "int32", 4, cap),
            "poses": _entry((cap, POSE_REFINE_DTYPE.itemsize // 8), "int64", 8, cap),
            "checks": _entry((cap, POSE_VERIFY_DTYPE.itemsize // 8), "int64", 8, cap),
            "keep": _entry((cap,), "uint8", 1, cap)}


class ExportedPoses(_Exported):
    """What DepthTemplates.pose_chain leaves on the GPU (lmx_pose_chain_on): torch tensors on the object's device, parallel to the
    clusters of the export they were computed from, valid for work queued on `stream` after the call --
      chain_header  int32 [8]       [0] n_live, [1] flags, [2] slots refined, [3] verified OK, [4] kept
      leaders       int32 [cap]     each cluster's leader, an index into the export's `matches`; -1: a dead slot or a broken list
      poses         int64 [cap, 17] lmx_pose_refine_t records (POSE_REFINE_DTYPE)
      checks        int64 [cap, 6]  lmx_pose_verify_t records (POSE_VERIFY_DTYPE)
      keep          uint8 [cap]     the erase rule of keep_verified
    Entries at or above n_live are not written.  Any other stream, or the host, synchronises with `stream` first; to_host() does."""

    NAMES = ("chain_header", "leaders", "poses", "checks", "keep")

    def __init__(self, cap_clusters, stream, device):
        lay = pose_chain_layout(cap_clusters)
        self.cap = lay["leaders"]["cap"]
        self._allocate(lay, stream, device)

    def _views(self):
        self.chain_header, self.leaders, self.poses, self.checks, self.keep = (self._backing[k] for k in self.NAMES)

    def _fits(self, caps):
        if self.cap < caps[1]:
            raise ValueError("out was made for %d clusters, the export holds up to %d" % (self.cap, caps[1]))

    def to_host(self):
        """Synchronises `stream` -> (chain_header int64 [8], leaders int32 [n_live], poses POSE_REFINE_DTYPE [n_live], checks
        POSE_VERIFY_DTYPE [n_live], keep bool [n_live])."""
        hdr, n = self._live()
        return (hdr, _records(self.leaders, n, np.int32), _records(self.poses, n, POSE_REFINE_DTYPE), _records(self.checks, n, POSE_VERIFY_DTYPE),
                _records(self.keep, n, np.uint8).astype(bool))


# lmx_rough_pose_t; status: the LMX_ROUGH_* values
ROUGH_POSE_DTYPE = np.dtype([("R", "<f8", (9,)), ("distance", "<f8"), ("D", "<f8"), ("ori_dist", "<f8"), ("x", "<i4"), ("y", "<i4"), ("n_members", "<i4"),
                             ("n_groups", "<i4"), ("group", "<i4"), ("n_group_members", "<i4"), ("front", "<i4"), ("center_hole", "<i4"), ("rect", "<i4", (4,)),
                             ("n_model", "<i4"), ("status", "<i4")])
ROUGH_NONE, ROUGH_OK, ROUGH_TOO_MANY_GROUPS, ROUGH_DEGENERATE, ROUGH_INVALID_VIEW, ROUGH_WINDOW_TOO_LARGE, ROUGH_EMPTY = range(7)
POSE_CHAIN_FLAG_ROUGH = 8          # chain_header[1] of lmx_rough_pose_chain_on: a slot ended with a rough status other than ROUGH_OK


def rough_trace_min(threshold_deg):
    """lmx_rough_trace_min: 1 + 2 cos(threshold) for a threshold inside (0, 180) degrees, what rough_pose_chain compares the trace of
    R_a^T R_b with."""
    out = C.c_double()
    _lib.check(_lib.lib().lmx_rough_trace_min(float(threshold_deg), C.byref(out)))
    return out.value


def rough_pose_layout(cap_clusters, cap_members):
    """The device arrays lmx_rough_pose_chain_on fills, as DepthTemplates.rough_pose_chain allocates them: pose_chain_layout's with `rough`
    in place of `leaders`, and member_group parallel to the export's members."""
    lay = pose_chain_layout(cap_clusters)
    cap, n_mem = lay["leaders"]["cap"], max(int(cap_members), 1)
    del lay["leaders"]
    lay["rough"] = _entry((cap, ROUGH_POSE_DTYPE.itemsize // 8), "int64", 8, cap)
    lay["member_group"] = _entry((n_mem,), "int32", 4, n_mem)
    return lay


class ExportedRoughPoses(_Exported):
    """What DepthTemplates.rough_pose_chain leaves on the GPU (lmx_rough_pose_chain_on): as ExportedPoses, with
      chain_header  int32 [8]       [0] n_live, [1] flags, [2] slots refined, [3] verified OK, [4] kept, [5] slots of status ROUGH_OK
      rough         int64 [cap, 19] lmx_rough_pose_t records (ROUGH_POSE_DTYPE)
      member_group  int32 [cap_members]  the orientation group of every member, parallel to the export's members
    in place of leaders."""
    NAMES = ("chain_header", "rough", "member_group", "poses", "checks", "keep")

    def __init__(self, cap_clusters, cap_members, stream, device):
        lay = rough_pose_layout(cap_clusters, cap_members)
        self.cap, self.cap_members = lay["rough"]["cap"], lay["member_group"]["cap"]
        self._allocate(lay, stream, device)

    def _views(self):
        self.chain_header, self.rough, self.member_group, self.poses, self.checks, self.keep = (self._backing[k] for k in self.NAMES)

    def _fits(self, caps):
        if self.cap < caps[1] or self.cap_members < caps[2]:
            raise ValueError("out was made for %d clusters and %d members, the export holds up to %d and %d" % (self.cap, self.cap_members, caps[1], caps[2]))

    def to_host(self):
        """Synchronises `stream` -> (chain_header int64 [8], rough ROUGH_POSE_DTYPE [n_live], member_group int32 [cap_members], poses
        POSE_REFINE_DTYPE [n_live], checks POSE_VERIFY_DTYPE [n_live], keep bool [n_live])."""
        hdr, n = self._live()
        return (hdr, _records(self.rough, n, ROUGH_POSE_DTYPE), _records(self.member_group, self.cap_members, np.int32), _records(self.poses, n, POSE_REFINE_DTYPE),
                _records(self.checks, n, POSE_VERIFY_DTYPE), _records(self.keep, n, np.uint8).astype(bool))


class PreparedBatch:
    """lmx_image descriptors of a batch of host frames, built once (the arrays are kept alive by this object)."""

    def __init__(self, frames):
        self.imgs, self.keep = _images(frames)
        self.n_frames, self.n_sources = len(frames), len(frames[0])

    def slice(self, first, count):
        """Frames [first, first + count) of this batch as a PreparedBatch of their own (shares the descriptors and the arrays)."""
        out = PreparedBatch.__new__(PreparedBatch)
        out.imgs = (_lib.Image * (count * self.n_sources)).from_address(C.addressof(self.imgs) + first * self.n_sources * C.sizeof(_lib.Image))
        out.keep = (self.imgs, self.keep)
        out.n_frames, out.n_sources = count, self.n_sources
        return out


class PreparedDeviceBatch(PreparedBatch):
    """The same for frames in device memory (device_images): what Detector.upload_device takes in place of the tensors when one batch is
    uploaded again and again (a decoder's ring of output surfaces, the rate script)."""

    def __init__(self, frames):
        self.imgs, self.keep = device_images(frames)
        self.n_frames, self.n_sources = len(frames), len(frames[0])


MESH_LIGHT = (0.35, -0.45, -0.82)   # the light direction of the mesh renderer's default camera


def _mesh_args(triangles, views, width, height, fx, fy, cx, cy, light):
    """-> (triangles float64 [n,3,3], lmx_mesh_camera, lmx_mesh_view array) for lmx_mesh_render / lmx_bank_train_mesh."""
    tri = np.ascontiguousarray(triangles, np.float64)
    if tri.ndim != 3 or tri.shape[1:] != (3, 3):
        raise TypeError("triangles must be [n, 3, 3] (metres, object frame)")
    cam = _lib.MeshCamera(int(width), int(height), float(fx), float(fy), width / 2.0 if cx is None else float(cx), height / 2.0 if cy is None else float(cy),
                          (C.c_double * 3)(*[float(v) for v in light]))
    packed = np.empty((len(views), 10), np.float64)
    for i, (R, dist) in enumerate(views):
        packed[i, :9] = np.asarray(R, np.float64).reshape(9)
        packed[i, 9] = dist
    return tri, cam, packed


def render_views(triangles, views, width=640, height=480, fx=826.119324, fy=826.119324, cx=None, cy=None, light=MESH_LIGHT, device=0):
    """lmx_mesh_render: the mesh (`triangles` [n,3,3], metres) seen from every (R [3,3], distance) of `views` with X_cam = R X_obj +
    (0, 0, distance) -> (gray u8 [n,H,W], depth u16 mm [n,H,W], mask u8 [n,H,W], rects int32 [n,4] (x, y, w, h))."""
    tri, cam, packed = _mesh_args(triangles, views, width, height, fx, fy, cx, cy, light)
    n = len(views)
    gray = np.empty((n, height, width), np.uint8)
    depth = np.empty((n, height, width), np.uint16)
    mask = np.empty((n, height, width), np.uint8)
    rects = np.zeros((n, 4), np.int32)
    _lib.check(_lib.lib().lmx_mesh_render(device, tri.ctypes.data, tri.shape[0], C.byref(cam), packed.ctypes.data_as(C.POINTER(_lib.MeshView)), n,
                                          gray.ctypes.data, depth.ctypes.data, mask.ctypes.data, rects.ctypes.data))
    return gray, depth, mask, rects


def _side_car_dict(p):
    """lmx_renderer_params -> dict of numpy arrays (copies) and the renderer_* scalars."""
    n = int(p.n_templates)
    arr = lambda ptr, shape, dt: (np.ctypeslib.as_array(ptr, shape=shape).astype(dt) if n else np.zeros(shape, dt))  # noqa: E731
    out = {"obj_origin_dists": arr(p.obj_origin_dists, (n,), np.float64), "rects": arr(p.rects, (n, 4), np.int32), "distances": arr(p.distances, (n,), np.float64),
           "R": arr(p.R, (n, 3, 3), np.float64), "T": arr(p.T, (n, 3), np.float64), "K": arr(p.K, (n, 3, 3), np.float64)}
    for k, _ in _lib.RendererParams._fields_[7:]:
        out[k] = getattr(p, k)
    return out


class NativeBank:
    """Owns an lmx_bank handle (host template state of cv::linemod::Detector)."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    @classmethod
    def from_bank(cls, bank: TemplateBank):
        L = _lib.lib()
        T = (C.c_int32 * len(bank.T))(*bank.T)
        mods = (_lib.ModalityDesc * len(bank.modalities))()
        for i, m in enumerate(bank.modalities):
            if m["type"] == "ColorGradient":
                mods[i] = _lib.ModalityDesc(_lib.LMX_MOD_COLOR_GRADIENT, m.get("weak_threshold", 10.0), m.get("strong_threshold", 55.0),
                                            m.get("num_features", 63), 0, 0, 0)
            elif m["type"] == "DepthNormal":
                mods[i] = _lib.ModalityDesc(_lib.LMX_MOD_DEPTH_NORMAL, 0.0, 0.0, m.get("num_features", 63),
                                            m.get("distance_threshold", 2000), m.get("difference_threshold", 50),
                                            m.get("extract_threshold", 2))
            else:
                raise ValueError("unknown modality %r" % (m["type"],))
        desc = _lib.BankDesc(len(bank.T), T, len(bank.modalities), mods)
        h = C.c_void_p()
        _lib.check(L.lmx_bank_create(C.byref(desc), C.byref(h)))
        self = cls(h.value)
        per = len(bank.T) * len(bank.modalities)
        for cid, templates, features in bank.classes:
            templates = np.ascontiguousarray(templates, np.int32)
            features = np.ascontiguousarray(features, np.int32)
            _lib.check(L.lmx_bank_add_class(self.h, cid.encode(), templates.shape[0] // per,
                                            templates.ctypes.data_as(C.POINTER(C.c_int32)),
                                            features.ctypes.data_as(C.POINTER(C.c_int32)), features.shape[0]))
        if getattr(bank, "normal_lut", None) is not None:
            self.set_normal_lut(bank.normal_lut)
        return self

    def set_normal_lut(self, lut):
        """DepthNormal's NORMAL_LUT[20][20][20] (upstream normal_lut.i); None = choose the default generator explicitly."""
        if lut is None:
            _lib.check(_lib.lib().lmx_bank_set_normal_lut(self.h, None))
        else:
            lut = np.ascontiguousarray(lut, np.uint8).reshape(_lib.LMX_NORMAL_LUT_SIZE)
            _lib.check(_lib.lib().lmx_bank_set_normal_lut(self.h, lut.ctypes.data))

    def load_normal_lut(self, path):
        _lib.check(_lib.lib().lmx_bank_load_normal_lut(self.h, str(path).encode()))

    def normal_lut(self):
        out = np.empty((20, 20, 20), np.uint8)
        _lib.check(_lib.lib().lmx_bank_get_normal_lut(self.h, out.ctypes.data))
        return out

    def normal_lut_origin(self):
        return int(_lib.lib().lmx_bank_normal_lut_origin(self.h))

    @classmethod
    def create(cls, T, modalities):
        """Empty bank: cv::linemod::Detector(modalities, T) as in the reference's trainers (src/renderer.cpp:179-185)."""
        return cls.from_bank(TemplateBank(T=list(T), modalities=list(modalities)))

    def add_template(self, sources, class_id, object_mask=None, device=0):
        """cv::linemod::Detector::addTemplate (reference src/renderer.cpp:308): -> (template_id or -1, bounding box (x, y, w, h))."""
        imgs, keep = _images([list(sources)])
        mask_img = None
        if object_mask is not None:
            m = object_mask
            if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1:
                raise TypeError("object_mask must be uint8 HxW")
            mask_img = _lib.Image(m.ctypes.data, m.shape[0], m.shape[1], 1, 1, m.strides[0])
        tid = C.c_int32(-1)
        bb = (C.c_int32 * 4)()
        _lib.check(_lib.lib().lmx_bank_add_template(self.h, device, imgs, len(sources), class_id.encode(),
                                                    C.byref(mask_img) if mask_img is not None else None, C.byref(tid), bb))
        del keep
        return tid.value, tuple(bb)

    def train_mesh(self, triangles, views, width=640, height=480, fx=826.119324, fy=826.119324, cx=None, cy=None, class_id="obj", light=MESH_LIGHT,
                   device=0, save_side_car=None, side_car_scalars=None, device_candidates=False):
        """lmx_bank_train_mesh, the reference's trainer loop (src/renderer.cpp:262-329): renders every (R, distance) of `views` on the
        device and adds a template per view addTemplate accepts, in view order.  -> list of dicts per ACCEPTED view {view, rect, distance}
        (what meshsynth.train_bank returns); `.last_template_ids` = int32 [n_views] (-1: rejected), `.last_side_car` = the renderer-params
        side-car of the accepted views as a dict (obj_origin_dists, rects, distances, R, T, K, renderer_*).  save_side_car: also write it
        as a *_renderer_params.yml, with `side_car_scalars` (renderer_n_points, renderer_radius_min, ...) set first.
        device_candidates: lmx_bank_train_mesh_opts with LMX_TRAIN_CANDIDATES_DEVICE -- the candidates of every window are found and
        compacted on the device and only their lists are read back; the result is the same.  `.last_train_stats` = the call's
        lmx_train_mesh_stats as a dict (n_views, n_accepted, n_device_views, n_fallback_views, n_candidates, list_bytes, total_ms,
        device_wait_ms, host_select_ms)."""
        tri, cam, packed = _mesh_args(triangles, views, width, height, fx, fy, cx, cy, light)
        ids = np.full(len(views), -1, np.int32)
        side = C.POINTER(_lib.RendererParams)()
        L = _lib.lib()
        opts = _lib.TrainMeshOpts(C.sizeof(_lib.TrainMeshOpts), _lib.LMX_TRAIN_CANDIDATES_DEVICE if device_candidates else _lib.LMX_TRAIN_CANDIDATES_HOST)
        stats = _lib.TrainMeshStats()
        self.last_train_stats = None
        _lib.check(L.lmx_bank_train_mesh_opts(self.h, device, tri.ctypes.data, tri.shape[0], C.byref(cam), packed.ctypes.data_as(C.POINTER(_lib.MeshView)),
                                              len(views), class_id.encode(), ids.ctypes.data, C.byref(side), C.byref(opts), C.byref(stats)))
        self.last_train_stats = {k: getattr(stats, k) for k, _ in _lib.TrainMeshStats._fields_}
        try:
            for k, v in (side_car_scalars or {}).items():
                setattr(side.contents, k, v)
            self.last_side_car = _side_car_dict(side.contents)
            if save_side_car is not None:
                _lib.check(L.lmx_renderer_params_save(side, str(save_side_car).encode()))
        finally:
            L.lmx_renderer_params_free(side)
        self.last_template_ids = ids
        sc = self.last_side_car
        acc = np.nonzero(ids >= 0)[0]
        return [{"view": int(v), "rect": tuple(int(x) for x in sc["rects"][k]), "distance": float(sc["obj_origin_dists"][k])} for k, v in enumerate(acc)]

    @classmethod
    def load_yaml(cls, path):
        h = C.c_void_p()
        _lib.check(_lib.lib().lmx_bank_load_yaml(str(path).encode(), C.byref(h)))
        return cls(h.value)

    def save_yaml(self, path):
        _lib.check(_lib.lib().lmx_bank_save_yaml(self.h, str(path).encode()))

    def to_bank(self) -> TemplateBank:
        L = _lib.lib()
        nl, nm = L.lmx_bank_pyramid_levels(self.h), L.lmx_bank_num_modalities(self.h)
        T = [L.lmx_bank_T(self.h, l) for l in range(nl)]
        mods = []
        for i in range(nm):
            d = _lib.ModalityDesc()
            _lib.check(L.lmx_bank_modality(self.h, i, C.byref(d)))
            if d.type == _lib.LMX_MOD_COLOR_GRADIENT:
                mods.append({"type": "ColorGradient", "weak_threshold": d.weak_threshold, "num_features": d.num_features,
                             "strong_threshold": d.strong_threshold})
            else:
                mods.append({"type": "DepthNormal", "distance_threshold": d.distance_threshold,
                             "difference_threshold": d.difference_threshold, "num_features": d.num_features,
                             "extract_threshold": d.extract_threshold})
        bank = TemplateBank(T=T, modalities=mods)
        if self.normal_lut_origin() in (_lib.LMX_LUT_USER, _lib.LMX_LUT_SIDECAR):
            bank.normal_lut = self.normal_lut()
        per = nl * nm
        for ci in range(L.lmx_bank_num_classes(self.h)):
            cid = L.lmx_bank_class_id(self.h, ci)
            n = L.lmx_bank_num_templates(self.h, cid)
            templates = np.zeros((n * per, 5), np.int32)
            feats = []
            fb = 0
            w, h, lv, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
            fp = C.POINTER(C.c_int32)()
            for t in range(n):
                for k in range(per):
                    _lib.check(L.lmx_bank_get_template(self.h, cid, t, k, C.byref(w), C.byref(h), C.byref(lv), C.byref(fp), C.byref(nf)))
                    templates[t * per + k] = (w.value, h.value, lv.value, fb, nf.value)
                    if nf.value:
                        feats.append(np.ctypeslib.as_array(fp, shape=(nf.value, 3)).copy())
                    fb += nf.value
            bank.classes.append((cid.decode(), templates, np.concatenate(feats, 0) if feats else np.zeros((0, 3), np.int32)))
        return bank

    def debug_tables(self, table, width, height, max_batch=1, shard_rank=0, shard_world=1, ls_flat=False):
        """Test hook (lmx_debug_bank_tables), no device needed: -> (bytes of table `table` (_lib.LMX_TAB_*) as a context with these
        parameters would upload it, as a uint8 array; the library's FNV-1a 64 of them)."""
        n, h = C.c_size_t(), C.c_uint64()
        args = (self.h, width, height, max_batch, shard_rank, shard_world, 1 if ls_flat else 0, table)
        _lib.check(_lib.lib().lmx_debug_bank_tables(*args, None, 0, C.byref(n), None))
        out = np.empty(n.value, np.uint8)
        _lib.check(_lib.lib().lmx_debug_bank_tables(*args, out.ctypes.data, out.nbytes, C.byref(n), C.byref(h)))
        return out, h.value

    def class_ids(self):
        L = _lib.lib()
        return [L.lmx_bank_class_id(self.h, i).decode() for i in range(L.lmx_bank_num_classes(self.h))]

    def __del__(self):
        try:
            if self.h:
                _lib.lib().lmx_bank_destroy(self.h)
                self.h = None
        except Exception:
            pass


def class_thresholds(bank_class_ids, thresholds, class_ids=()):
    """Per-class thresholds given as a mapping class id -> float, for the `..._thresholds` entry points: -> (float array with one entry
    per class of the bank, in class-index order; class-id array; its length).  The classes matched are those of `class_ids` (in that
    order) that the mapping holds, or, without `class_ids`, the mapping's keys in sorted order -- the order cv::linemod::Detector::match
    visits its class map in.  Classes absent from the mapping are not matched; a key the bank does not know is an error, and so is a
    call that would match no class at all."""
    known = list(bank_class_ids)
    unknown = [k for k in thresholds if k not in known]
    if unknown:
        raise ValueError("thresholds for classes the bank does not hold: %s" % unknown)
    visit = [c for c in (class_ids if len(class_ids) else sorted(thresholds, key=lambda s: s.encode())) if c in thresholds]
    if not visit:
        raise ValueError("no class to match: the threshold mapping holds none of the classes asked for")
    arr = (C.c_float * len(known))(*[float(thresholds.get(c, 0.0)) for c in known])   # entries of unmatched classes are never read
    cids = (C.c_char_p * len(visit))(*[c.encode() for c in visit])
    return arr, cids, len(visit)


def _cluster_params(vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh):
    return _lib.ClusterParams(int(vote_row_col_step), float(renderer_radius_min), float(renderer_radius_step), int(cluster_size_thresh))


def _side_car(obj_origin_dists, rects):
    """A side-car's per-template arrays -> (float64 [n], int32 [n, 4])."""
    return np.ascontiguousarray(obj_origin_dists, np.float64).reshape(-1), np.ascontiguousarray(rects, np.int32).reshape(-1, 4)


def _class_base(class_base):
    """The cumulative template counts of the classes joined in one DepthTemplates -> int32 [n_classes + 1]."""
    base = np.ascontiguousarray(class_base, np.int32).reshape(-1)
    if len(base) < 2:
        raise ValueError("class_base must hold one entry per class plus one")
    return base


def _collect_buffers(n_frames, cap_total, names):
    """The host lists of one collect_clusters* call and their cut per frame.  names: the result tuple in order, of _LIST_DTYPES' keys --
    "m", "d", "nd" parallel to the matches, "cl", "cc" to the clusters, "mem" flat and returned whole -- or None for a list this call has
    not.  -> (name -> address of a list of cap_total elements, with "mo" / "co", the size_t [n_frames + 1] offsets of the two families,
    which the library fills; cut() -> list per frame of the tuple, each range a copy)."""
    b = {k: np.zeros(cap_total, _LIST_DTYPES[k]) for k in names if k}
    ptr = {k: a.ctypes.data for k, a in b.items()}
    ptr["mo"], ptr["co"] = (C.c_size_t * (n_frames + 1))(), (C.c_size_t * (n_frames + 1))()

    def cut():
        offs = {k: ptr["co"] if k in ("cl", "cc") else ptr["mo"] for k in b}
        return [tuple(None if k is None else b[k] if k == "mem" else b[k][offs[k][f]:offs[k][f + 1]].copy() for k in names) for f in range(n_frames)]
    return ptr, cut


class Detector:
    """Device-resident detector: a template bank (or one rank's shard of it) in HBM plus per-frame workspaces.

    Mirrors cv::linemod::Detector for the matching side.  `match` is the drop-in for the call in
    rgbdDetector::linemod_detection (/root/reference/src/rgbdDetector.cpp:33)."""

    def __init__(self, bank, width, height, device=0, max_batch=1, max_candidates=0, shard_rank=0, shard_world=1, stream=None, hipgraph=False, overlap=False,
                 async_input=False, gray=False):
        if isinstance(bank, TemplateBank):
            self.native_bank = NativeBank.from_bank(bank)
            self.bank = bank
        elif isinstance(bank, NativeBank):
            self.native_bank = bank
            self.bank = bank.to_bank()
        else:
            raise TypeError("bank must be a TemplateBank or NativeBank")
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, int(device)
        # gray (LMX_CTX_GRAY): ColorGradient sources are uint8 HxW (a MONO8 frame) instead of HxWx3; matches equal those of the frame copied into B, G, R
        self.gray = bool(gray)
        desc = _lib.CtxDesc(device, width, height, max_batch, max_candidates, shard_rank, shard_world, stream,
                            (1 if hipgraph else 0) | (2 if overlap else 0) | (4 if async_input else 0) | (_lib.LMX_CTX_GRAY if gray else 0))
        self.h = C.c_void_p()
        _lib.check(_lib.lib().lmx_ctx_create(self.native_bank.h, C.byref(desc), C.byref(self.h)))
        self._class_ids = self.native_bank.class_ids()
        self.max_outstanding = int(_lib.lib().lmx_ctx_max_outstanding(self.h))   # enqueues that may be in flight before a collect

    # ---- cv::linemod::Detector-style accessors -----------------------------------------------------------
    @classmethod
    def readLinemod(cls, filename, width, height, **kw):
        return cls(NativeBank.load_yaml(filename), width, height, **kw)

    def classIds(self):
        return list(self._class_ids)

    def numTemplates(self, class_id=None):
        return _lib.lib().lmx_bank_num_templates(self.native_bank.h, class_id.encode() if class_id else None)

    def getTemplates(self, class_id, template_id):
        return self.bank.get_templates(class_id, template_id)

    def getT(self, level):
        return self.bank.T[level]

    def pyramidLevels(self):
        return self.bank.pyramid_levels

    # ---- matching -------------------------------------------------------------------------------------------
    @staticmethod
    def _cids(class_ids):
        n = len(class_ids)
        arr = (C.c_char_p * max(1, n))(*[c.encode() for c in class_ids])
        return arr, n

    def match(self, sources, threshold, class_ids=(), cap=1 << 14):
        """One frame through `lmx_match`, the drop-in for Detector::match.  Returns MATCH_DTYPE records in upstream
        output order (std::sort + std::unique applied).  `threshold`: a float, or a mapping class id -> float (per-class thresholds,
        see class_thresholds); the same holds for match_masked, match_batch and enqueue."""
        L = _lib.lib()
        imgs, keep = _images([sources])
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_size_t()
        if isinstance(threshold, Mapping):
            thr, cids, ncid = class_thresholds(self._class_ids, threshold, class_ids)
            _lib.check(L.lmx_match_thresholds(self.h, imgs, len(sources), thr, len(thr), cids, ncid, out.ctypes.data, cap, C.byref(n)))
            del keep
            return out[:n.value].copy()
        cids, ncid = self._cids(class_ids)
        _lib.check(L.lmx_match(self.h, imgs, len(sources), C.c_float(threshold), cids, ncid, out.ctypes.data, cap, C.byref(n)))
        del keep
        return out[:n.value].copy()

    def match_masked(self, sources, masks, threshold, class_ids=(), cap=1 << 14):
        """Detector::match(sources, threshold, matches, class_ids, noArray(), masks): masks = one uint8 HxW array per modality (None
        entries = no mask for that source)."""
        imgs, keep = _images([sources])
        marr = (_lib.Image * len(sources))()
        for i, m in enumerate(masks):
            if m is None:
                marr[i] = _lib.Image(None, 0, 0, 1, 1, 0)
            else:
                if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1:
                    raise TypeError("masks must be uint8 HxW")
                marr[i] = _lib.Image(m.ctypes.data, m.shape[0], m.shape[1], 1, 1, m.strides[0])
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_size_t()
        if isinstance(threshold, Mapping):
            thr, cids, ncid = class_thresholds(self._class_ids, threshold, class_ids)
            _lib.check(_lib.lib().lmx_match_masked_thresholds(self.h, imgs, marr, len(sources), thr, len(thr), cids, ncid, out.ctypes.data, cap, C.byref(n)))
            del keep
            return out[:n.value].copy()
        cids, ncid = self._cids(class_ids)
        _lib.check(_lib.lib().lmx_match_masked(self.h, imgs, marr, len(sources), C.c_float(threshold), cids, ncid, out.ctypes.data, cap, C.byref(n)))
        del keep
        return out[:n.value].copy()

    def upload_masks(self, masks):
        """masks: list (per frame of the most recent upload) of list (per modality) of uint8 HxW arrays or None."""
        flat = [m for fr in masks for m in fr]
        marr = (_lib.Image * len(flat))()
        for i, m in enumerate(flat):
            marr[i] = _lib.Image(None, 0, 0, 1, 1, 0) if m is None else _lib.Image(m.ctypes.data, m.shape[0], m.shape[1], 1, 1, m.strides[0])
        _lib.check(_lib.lib().lmx_ctx_upload_masks(self.h, len(masks), marr, len(masks[0])))

    def match_prepared(self, batch, threshold, cap=1 << 12):
        """`lmx_match` on a one-frame PreparedBatch: the lmx_image descriptors were built once (what a C++ caller holding cv::Mat
        headers passes), so the call costs what the library costs, not the marshalling."""
        if getattr(self, "_mp_out", None) is None or len(self._mp_out) < cap:
            self._mp_out = np.zeros(cap, MATCH_DTYPE)
            self._mp_n = C.c_size_t()
            self._mp_cids = (C.c_char_p * 1)()
        _lib.check(_lib.lib().lmx_match(self.h, batch.imgs, batch.n_sources, C.c_float(threshold), self._mp_cids, 0, self._mp_out.ctypes.data, cap, C.byref(self._mp_n)))
        return self._mp_out[:self._mp_n.value].copy()

    def match_batch(self, frames, threshold, class_ids=(), cap=1 << 12):
        """n frames through `lmx_match_batch` (per-frame output capacity `cap`)."""
        L = _lib.lib()
        imgs, keep = _images(frames)
        out = np.zeros((len(frames), cap), MATCH_DTYPE)
        n_out = (C.c_size_t * len(frames))()
        if isinstance(threshold, Mapping):
            thr, cids, ncid = class_thresholds(self._class_ids, threshold, class_ids)
            _lib.check(L.lmx_match_batch_thresholds(self.h, len(frames), imgs, len(frames[0]), thr, len(thr), cids, ncid, out.ctypes.data, cap, n_out))
        else:
            cids, ncid = self._cids(class_ids)
            _lib.check(L.lmx_match_batch(self.h, len(frames), imgs, len(frames[0]), C.c_float(threshold), cids, ncid,
                                         out.ctypes.data, cap, n_out))
        del keep
        return [out[f, :n_out[f]].copy() for f in range(len(frames))]

    # split-phase API
    def upload(self, frames):
        """frames: list (per frame) of list (per modality) of numpy arrays, or a batch prepared once with `prepare_batch` (a caller
        that uploads the same host buffers repeatedly -- a camera ring, the bench -- skips rebuilding the lmx_image descriptors)."""
        if isinstance(frames, PreparedBatch):
            _lib.check(_lib.lib().lmx_ctx_upload(self.h, frames.n_frames, frames.imgs, frames.n_sources))
            return
        imgs, keep = _images(frames)
        _lib.check(_lib.lib().lmx_ctx_upload(self.h, len(frames), imgs, len(frames[0])))
        del keep

    @staticmethod
    def prepare_batch(frames):
        return PreparedBatch(frames)

    def upload_wait(self):
        """Host-side wait for the most recent upload's transfer (needed only with async_input and pinned sources)."""
        _lib.check(_lib.lib().lmx_ctx_upload_wait(self.h))

    def upload_raw(self, frames, src_size, crop_xy=(0, 0), blur3=True, mono=False, depth_float_m=False):
        """Raw camera frames + the node-side steps in front of match() on the device (lmx_ctx_upload_raw): optional
        MONO8->BGR, GaussianBlur 3x3 on the full frame, crop to the context size, float-metre depth -> u16 mm."""
        pre = _lib.PreDesc(src_size[0], src_size[1], crop_xy[0], crop_xy[1], int(blur3), int(mono), int(depth_float_m))
        if isinstance(frames, PreparedBatch):   # descriptors built once (a camera ring, the bench)
            _lib.check(_lib.lib().lmx_ctx_upload_raw(self.h, frames.n_frames, frames.imgs, frames.n_sources, C.byref(pre)))
            return
        imgs, keep = _images(frames)
        _lib.check(_lib.lib().lmx_ctx_upload_raw(self.h, len(frames), imgs, len(frames[0]), C.byref(pre)))
        del keep

    def upload_device(self, frames, src_size=None, crop_xy=(0, 0), blur3=False, mono=False, depth_float_m=False, stream=None):
        """Frames that already live in this context's GPU memory (lmx_ctx_upload_device): list (per frame) of list (per modality) of torch
        tensors or objects with __cuda_array_interface__ (device_images); nothing passes through the host.  src_size=None: frame-sized
        sources copied as they are; with src_size=(width, height) the node-side steps of upload_raw (crop, blur3, mono, depth_float_m)
        run on the way.  The sources are read behind what `stream` (default: the tensors' current torch stream, else the null stream)
        holds at the call, and that stream then waits for the ingest: the tensors may be overwritten or freed on it right away.
        `frames` may be a batch prepared once with prepare_device_batch."""
        if isinstance(frames, PreparedDeviceBatch):     # descriptors built once (Detector.prepare_device_batch)
            imgs, keep, n_frames, n_sources = frames.imgs, frames.keep, frames.n_frames, frames.n_sources
        else:
            imgs, keep = device_images(frames)
            n_frames, n_sources = len(frames), len(frames[0])
        pre = None if src_size is None else C.byref(_lib.PreDesc(src_size[0], src_size[1], crop_xy[0], crop_xy[1], int(blur3), int(mono), int(depth_float_m)))
        _lib.check(_lib.lib().lmx_ctx_upload_device(self.h, n_frames, imgs, n_sources, pre, _device_stream(keep, stream)))
        del keep

    @staticmethod
    def prepare_device_batch(frames):
        return PreparedDeviceBatch(frames)

    def enqueue(self, n_frames, threshold, class_ids=()):
        if isinstance(threshold, Mapping):
            thr, cids, ncid = class_thresholds(self._class_ids, threshold, class_ids)
            _lib.check(_lib.lib().lmx_ctx_enqueue_thresholds(self.h, n_frames, thr, len(thr), cids, ncid))
            return
        cids, ncid = self._cids(class_ids)
        _lib.check(_lib.lib().lmx_ctx_enqueue(self.h, n_frames, C.c_float(threshold), cids, ncid))

    def collect(self, n_frames, cap_total=1 << 16):
        """-> list (per frame) of MATCH_DTYPE arrays in upstream output order (views into a reused buffer are copied)."""
        if getattr(self, "_flat", None) is None or len(self._flat) < cap_total:
            self._flat = np.zeros(cap_total, MATCH_DTYPE)
        offs = (C.c_size_t * (n_frames + 1))()
        _lib.check(_lib.lib().lmx_ctx_collect_flat(self.h, n_frames, self._flat.ctypes.data, len(self._flat), offs))
        return [self._flat[offs[f]:offs[f + 1]].copy() for f in range(n_frames)]

    def set_cluster_sidecar(self, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh=2):
        """Side-car of the device-side consumer chain (lmx_ctx_set_cluster_sidecar): per-template origin distances and rects."""
        d, r = _side_car(obj_origin_dists, rects)
        pp = _cluster_params(vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh)
        _lib.check(_lib.lib().lmx_ctx_set_cluster_sidecar(self.h, d.ctypes.data, r.ctypes.data, len(d), C.byref(pp)))

    def collect_clusters(self, n_frames, cap_total=1 << 16):
        """Device-side std::sort + std::unique + rcd_voting/filter/scoring/IoU-NMS on the oldest outstanding enqueue
        (lmx_ctx_collect_clusters) -> list per frame of (matches, clusters, members)."""
        p, cut = _collect_buffers(n_frames, cap_total, ("m", "cl", "mem"))
        _lib.check(_lib.lib().lmx_ctx_collect_clusters(self.h, n_frames, p["m"], cap_total, p["mo"], p["cl"], cap_total, p["co"], p["mem"], cap_total))
        return cut()

    def collect_clusters_depth(self, n_frames, templates, class_index=-1, no_value=-np.inf, cap_total=1 << 16):
        """collect_clusters with the clusters ranked by the depth score (lmx_ctx_collect_clusters_depth): `templates` is a DepthTemplates
        whose upload_scene(depth_frames) was called after the enqueue.  -> list per frame of (matches, diffs, clusters, members), equal
        to collect + templates.diff + cluster_matches_scored(depth_values(diffs)) bit for bit; no_value is what a match with nothing to
        compare contributes to its cluster's mean."""
        p, cut = _collect_buffers(n_frames, cap_total, ("m", "d", "cl", "mem"))
        _lib.check(_lib.lib().lmx_ctx_collect_clusters_depth(self.h, n_frames, templates.h, int(class_index), float(no_value), p["m"], cap_total, p["mo"],
                                                             p["d"], p["cl"], cap_total, p["co"], p["mem"], cap_total))
        return cut()

    def collect_clusters_depth_normal(self, n_frames, templates, class_index=-1, no_value=-np.inf, cap_total=1 << 16):
        """collect_clusters_depth with the normal term in the score (lmx_ctx_collect_clusters_depth_normal): `templates` is a DepthTemplates
        after enable_normals whose upload_scene(depth_frames) was called after the enqueue.  -> list per frame of (matches, diffs, ndiffs,
        clusters, members), equal to collect + templates.normal_diff + cluster_matches_scored(normal_values(diffs, ndiffs)) bit for bit.
        exp(score) is the reference's getClusterScore when every member has something to compare."""
        p, cut = _collect_buffers(n_frames, cap_total, ("m", "d", "nd", "cl", "mem"))
        _lib.check(_lib.lib().lmx_ctx_collect_clusters_depth_normal(self.h, n_frames, templates.h, int(class_index), float(no_value), p["m"], cap_total,
                                                                    p["mo"], p["d"], p["nd"], p["cl"], cap_total, p["co"], p["mem"], cap_total))
        return cut()

    def set_cluster_sidecar_class(self, class_index, obj_origin_dists, rects, vote_row_col_step=1, renderer_radius_min=0.0, renderer_radius_step=1.0,
                                  cluster_size_thresh=2):
        """Class class_index's side-car of the per-class device chain (lmx_ctx_set_cluster_sidecar_class), class_index 0 .. 15; empty
        obj_origin_dists remove it.  The un-classed side-car of set_cluster_sidecar is separate state."""
        d, r = _side_car(obj_origin_dists, rects)
        if len(r) != len(d):
            raise ValueError("one rect per origin distance")
        pp = _cluster_params(vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh)
        _lib.check(_lib.lib().lmx_ctx_set_cluster_sidecar_class(self.h, int(class_index), d.ctypes.data if len(d) else None, r.ctypes.data if len(d) else None,
                                                                len(d), C.byref(pp)))

    def collect_clusters_classes(self, n_frames, templates=None, class_base=None, normals=False, no_value=-np.inf, cap_total=1 << 16):
        """collect_clusters for a bank of several classes (lmx_ctx_collect_clusters_classes): votes, filters, scores and suppresses per class
        with the side-cars of set_cluster_sidecar_class.  -> list per frame of (matches, diffs, ndiffs, clusters, cluster_class, members);
        a frame's clusters are class 0's, then class 1's, ..., cluster_class names each one's class.  templates None: mean similarity, diffs
        and ndiffs are None.  Else `templates` is a DepthTemplates holding all classes' crops (DepthTemplates.append), class c's at
        class_base[c]:class_base[c + 1], whose upload_scene was called after the enqueue; normals adds the normal term (ndiffs is None
        without).  Equal to collect + per-class diffs + cluster_matches_classes bit for bit; not to two single-class detectors, whose std::unique
        may keep other templates of a duplicate (include/lmx.h)."""
        score, scored = None, templates is not None
        if scored:
            base = _class_base(class_base)
            score = C.byref(_lib.ClassScore(templates.h, base.ctypes.data, len(base) - 1, int(bool(normals)), float(no_value)))
        p, cut = _collect_buffers(n_frames, cap_total, ("m", "d" if scored else None, "nd" if scored and normals else None, "cl", "cc", "mem"))
        _lib.check(_lib.lib().lmx_ctx_collect_clusters_classes(self.h, n_frames, score, p["m"], cap_total, p["mo"], p.get("d"), p.get("nd"), p["cl"], p["cc"],
                                                               cap_total, p["co"], p["mem"], cap_total))
        return cut()

    def raw_matches_ptrs(self):
        rec, cnt, cap = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _lib.check(_lib.lib().lmx_ctx_raw_matches(self.h, C.byref(rec), C.byref(cnt), C.byref(cap)))
        return rec.value, cnt.value, cap.value

    def export_raw(self, d_block_ptr, capacity_records):
        """One D2D copy of this context's gather block (64-byte header + capacity_records x 32 B) on the context's stream."""
        _lib.check(_lib.lib().lmx_ctx_export_raw(self.h, d_block_ptr, capacity_records))

    def export_raw_on(self, d_block_ptr, capacity_records, stream):
        """The same copy on `stream` (a raw hipStream_t), which first waits on the device for the most recent enqueue."""
        _lib.check(_lib.lib().lmx_ctx_export_raw_on(self.h, d_block_ptr, capacity_records, stream))

    def export_matches(self, n_frames, clusters=False, oldest=False, max_large_frames=0, cap_matches=1 << 16, cap_clusters=4096, cap_members=1 << 16,
                       stream=None, out=None):
        """The final matches of an enqueue -- and with clusters=True the clusters and members of collect_clusters -- left in GPU memory
        (lmx_ctx_export_matches_on) -> ExportedMatches.  The most recent enqueue, or with oldest=True the oldest outstanding one; it stays
        outstanding (release() or a collect ends it).  max_large_frames: frames of 2049 .. 16384 raw records this call may finish (2.4 MB of
        workspace each); the others get status 1 and can go through collect.  Nothing waits on the host: the results are valid for work
        queued afterwards on `stream` (a torch stream or a raw hipStream_t; default: the current torch stream of the context's device).
        out: an ExportedMatches of an earlier call with the same n_frames and clusters, written again in place of fresh tensors (its
        stream is used unless `stream` is given); the capacities are then the smaller of the arguments' and its own."""
        stream = _torch_stream(stream, out.stream if out is not None else None, self.device)
        out, caps = ExportedMatches._fresh_or(out, (n_frames, bool(clusters)), (cap_matches, cap_clusters, cap_members), stream, self.device)
        t = out._backing
        desc = _lib.ExportDesc(C.sizeof(_lib.ExportDesc), int(bool(oldest)), int(bool(clusters)), int(max_large_frames), t["header"].data_ptr(),
                               t["frame_info"].data_ptr(), t["matches"].data_ptr(), caps[0], t["clusters"].data_ptr() if clusters else None, caps[1],
                               t["members"].data_ptr() if clusters else None, caps[2])
        _lib.check(_lib.lib().lmx_ctx_export_matches_on(self.h, n_frames, C.byref(desc), int(stream.cuda_stream)))
        return out

    def export_clusters(self, n_frames, templates=None, class_index=-1, normals=False, no_value=-np.inf, classes=False, class_base=None, oldest=False,
                        max_large_frames=0, cap_matches=1 << 16, cap_clusters=4096, cap_members=1 << 16, stream=None, out=None):
        """export_matches(clusters=True) for every cluster chain (lmx_ctx_export_clusters_on) -> ExportedClusters.  templates None: mean
        similarity; a DepthTemplates whose upload_scene / upload_scene_device was called after the enqueue: the depth score, with
        normals=True (after enable_normals) depth + normal.  classes=True: the per-class chain with the side-cars of
        set_cluster_sidecar_class; with templates it also takes class_base as collect_clusters_classes does (class_index is then not
        used).  Equal, for every delivered frame, to collect_clusters / _depth / _depth_normal / _classes of the same enqueue, which
        stays outstanding.  Nothing waits on the host; the first scored call allocates 16 bytes per record the slot can hold
        (max_batch x max_candidates; twice with normals).  stream, out, oldest, max_large_frames and the capacities as export_matches (diffs / ndiffs share cap_matches,
        cluster_class cap_clusters)."""
        score = 0 if templates is None else (2 if normals else 1)
        stream = _torch_stream(stream, out.stream if out is not None else None, self.device)
        out, caps = ExportedClusters._fresh_or(out, (n_frames, score, bool(classes)), (cap_matches, cap_clusters, cap_members), stream, self.device)
        base, n_classes = None, 0
        if classes and score:
            base = _class_base(class_base)
            n_classes = len(base) - 1
        t = out._backing
        ptr = lambda k: t[k].data_ptr() if k in t else None   # noqa: E731
        desc = _lib.ExportClustersDesc(C.sizeof(_lib.ExportClustersDesc), int(bool(oldest)), int(max_large_frames), int(bool(classes)), score,
                                       int(class_index), n_classes, 0, templates.h if score else None, base.ctypes.data if base is not None else None,
                                       float(no_value), ptr("header"), ptr("frame_info"), ptr("matches"), caps[0], ptr("diffs"), ptr("ndiffs"),
                                       ptr("clusters"), caps[1], ptr("cluster_class"), ptr("members"), caps[2])
        _lib.check(_lib.lib().lmx_ctx_export_clusters_on(self.h, n_frames, C.byref(desc), int(stream.cuda_stream)))
        return out

    def release(self):
        """Drop the oldest outstanding enqueue without a read-back (its records were consumed on the device)."""
        _lib.check(_lib.lib().lmx_ctx_release(self.h))

    def sync(self):
        _lib.check(_lib.lib().lmx_ctx_sync(self.h))

    # ---- introspection ---------------------------------------------------------------------------------------
    def level_shape(self, level):
        return self.height >> level, self.width >> level

    def debug_quantized(self, frame, level, modality):
        H, W = self.level_shape(level)
        out = np.empty((H, W), np.uint8)
        _lib.check(_lib.lib().lmx_ctx_debug_read(self.h, frame, _lib.LMX_DBG_QUANTIZED, level, modality, out.ctypes.data, out.nbytes))
        return out

    def debug_linear_memory(self, frame, level, modality):
        H, W = self.level_shape(level)
        T = self.bank.T[level]
        out = np.empty((8, T * T, (H // T) * (W // T)), np.uint8)
        _lib.check(_lib.lib().lmx_ctx_debug_read(self.h, frame, _lib.LMX_DBG_LINEAR_MEMORY, level, modality, out.ctypes.data, out.nbytes))
        return out

    def debug_raw(self, what, nbytes, level=0, modality=0):
        """Test hook: a whole device allocation as it is, pads and tails included, as nbytes uint8 (what = _lib.LMX_DBG_RAW_SPREAD of
        (level, modality), LMX_DBG_RAW_NIBBLES, or LMX_DBG_RAW_BYTES of modality; include/lmx.h gives the sizes, which the caller works out
        from the geometry in NativeBank.debug_tables' summary).  Too few bytes are refused, and the error names the size."""
        out = np.empty(int(nbytes), np.uint8)
        _lib.check(_lib.lib().lmx_ctx_debug_read(self.h, 0, int(what), level, modality, out.ctypes.data, out.nbytes))
        return out

    def debug_depth(self, frame, modality):
        out = np.empty((self.height, self.width), np.uint16)
        _lib.check(_lib.lib().lmx_ctx_debug_read(self.h, frame, 3, 0, modality, out.ctypes.data, out.nbytes))
        return out

    def debug_pyramid_bgr(self, frame, level, modality=0):
        """Colour source of pyramid level `level`: (H_l, W_l, 3), or (H_l, W_l) on a gray detector."""
        H, W = self.level_shape(level)
        out = np.empty((H, W) if self.gray else (H, W, 3), np.uint8)
        _lib.check(_lib.lib().lmx_ctx_debug_read(self.h, frame, _lib.LMX_DBG_PYRAMID_BGR, level, modality, out.ctypes.data, out.nbytes))
        return out

    def debug_enqueue_labels(self, labels, threshold=None, thresholds=None, class_ids=()):
        """Test hook (lmx_ctx_debug_enqueue_labels): an enqueue whose chain starts at the label images.  labels[level][modality] is a uint8
        array [n_frames, H_l, W_l] (level_shape) that becomes the context's label image as it is; spread, scoring, refinement and read-back
        then run as enqueue(n_frames, threshold) -- or, with `thresholds` (a mapping class id -> threshold), as the per-class enqueue --
        launches them.  No upload is needed; collect / collect_clusters* / stats follow as after enqueue."""
        L, M = len(self.bank.T), len(self.bank.modalities)
        if len(labels) != L or any(len(p) != M for p in labels):
            raise ValueError("labels: %d levels x %d modalities expected" % (L, M))
        if (threshold is None) == (thresholds is None):
            raise ValueError("give either threshold (a float) or thresholds (a mapping class id -> float)")
        n_frames = int(np.shape(labels[0][0])[0]) if np.ndim(labels[0][0]) == 3 else 0
        flat = []
        for l, per_level in enumerate(labels):
            for a in per_level:
                a = np.ascontiguousarray(a, np.uint8)
                if a.shape != (n_frames,) + tuple(self.level_shape(l)):
                    raise ValueError("labels of level %d: shape %s, expected %s" % (l, a.shape, (n_frames,) + tuple(self.level_shape(l))))
                flat.append(a)
        ptrs = (C.c_void_p * len(flat))(*[a.ctypes.data for a in flat])
        # read by the stream's copies: kept while the call can still be outstanding
        self._label_keep = (getattr(self, "_label_keep", None) or []) + [flat]
        del self._label_keep[:-max(1, self.max_outstanding)]
        if thresholds is not None:
            thr, cids, ncid = class_thresholds(self._class_ids, thresholds, class_ids)
            _lib.check(_lib.lib().lmx_ctx_debug_enqueue_labels(self.h, n_frames, ptrs, len(flat), C.c_float(0.0), thr, len(thr), cids, ncid))
            return
        cids, ncid = self._cids(class_ids)
        _lib.check(_lib.lib().lmx_ctx_debug_enqueue_labels(self.h, n_frames, ptrs, len(flat), C.c_float(threshold), None, 0, cids, ncid))

    def stats(self):
        a, b = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().lmx_ctx_stats(self.h, C.byref(a), C.byref(b)))
        return {"candidates": a.value, "raw_matches": b.value}

    def launch_helper_counters(self):
        """Test hook (lmx_debug_launch_helper_counters): the helper thread of the one-frame call with host frames -- jobs it ran, times it went
        to sleep, wake-ups it was sent, and `awake` = jobs - notifies, the calls that found it still spinning.  All zero before the first such call."""
        k = (C.c_uint64 * 3)()
        _lib.check(_lib.lib().lmx_debug_launch_helper_counters(self.h, k))
        return {"jobs": int(k[0]), "sleeps": int(k[1]), "notifies": int(k[2]), "awake": int(k[0]) - int(k[2])}

    def chain_stats(self):
        """Which path completed the frames of the last collect_clusters* call (lmx_ctx_chain_stats): frames, frames_lds (at most F2_MAX raw
        records), frames_large (up to F2_LARGE_MAX, the large-frame kernel), frames_host_records, frames_host_other (side-car / ring range),
        max_frame_records (largest raw count among the frames beyond F2_MAX; 0: none) and large_workspace_bytes."""
        s = _lib.ChainStats()
        _lib.check(_lib.lib().lmx_ctx_chain_stats(self.h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in _lib.ChainStats._fields_}

    def set_profiling(self, on=True):
        """on: True = every kernel, False = none, or a kernel name / list of names (only those get HIP events)."""
        L = _lib.lib()
        if on is True:
            mask = -1
        elif not on:
            mask = 0
        else:
            names = [on] if isinstance(on, str) else list(on)
            ids = {L.lmx_kernel_name(k).decode(): k for k in range(L.lmx_num_kernels())}
            mask = 0
            for n in names:
                mask |= 1 << ids[n]
        _lib.check(L.lmx_ctx_set_profiling(self.h, mask))

    def reset_profiling(self):
        _lib.check(_lib.lib().lmx_ctx_reset_profiling(self.h))

    def kernel_times(self):
        L = _lib.lib()
        out = {}
        for k in range(L.lmx_num_kernels()):
            ms, n = C.c_double(), C.c_int64()
            _lib.check(L.lmx_ctx_kernel_time(self.h, k, C.byref(ms), C.byref(n)))
            out[L.lmx_kernel_name(k).decode()] = (ms.value, n.value)
        return out

    def device_kernel_name(self, kernel_name):
        """Name of the device kernel a profiler shows for this context's `kernel_name` (e.g. k_score_coarse -> k_score_coarse_u8)."""
        L = _lib.lib()
        for k in range(L.lmx_num_kernels()):
            if L.lmx_kernel_name(k).decode() == kernel_name:
                return L.lmx_ctx_device_kernel_name(self.h, k).decode()
        raise KeyError(kernel_name)

    def algorithmic_bytes(self, kernel_name, n_frames):
        L = _lib.lib()
        for k in range(L.lmx_num_kernels()):
            if L.lmx_kernel_name(k).decode() == kernel_name:
                v = C.c_double()
                _lib.check(L.lmx_ctx_algorithmic_bytes(self.h, k, n_frames, C.byref(v)))
                return v.value
        raise KeyError(kernel_name)

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().lmx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedArena:
    """Pinned host memory (lmx_host_alloc == hipHostMalloc) handed out as numpy arrays: frames placed here take the zero-copy
    upload path (DMA straight from the caller's buffer, no staging copy)."""

    def __init__(self, nbytes):
        self.p = C.c_void_p()
        _lib.check(_lib.lib().lmx_host_alloc(nbytes, C.byref(self.p)))
        self.nbytes, self.used = nbytes, 0
        self._buf = (C.c_uint8 * nbytes).from_address(self.p.value)

    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        off = (self.used + 255) & ~255
        if off + n > self.nbytes:
            raise MemoryError("PinnedArena exhausted")
        self.used = off + n
        return np.frombuffer(self._buf, dtype=dtype, count=int(np.prod(shape)), offset=off).reshape(shape)

    def put(self, a):
        out = self.empty(a.shape, a.dtype)
        out[...] = a
        return out

    def close(self):
        if getattr(self, "p", None) and self.p.value:
            self._buf = None
            _lib.lib().lmx_host_free(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _cluster_outputs(n_matches):
    """What the cluster_matches* calls write -> (clusters CLUSTER_DTYPE and members int32, each with room for every match; the size_t
    the library leaves the number of clusters in)."""
    n = max(1, n_matches)
    return np.zeros(n, CLUSTER_DTYPE), np.zeros(n, np.int32), C.c_size_t()


def cluster_matches(matches, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh=2):
    """rcd_voting -> cluster_filter -> cluster_scoring -> nonMaximaSuppressionUsingIOU on one frame's matches
    (reference: src/linemod_ensenso_detect_3_mult_detect_service.cpp:376-447).  Returns (clusters, members): clusters is a
    CLUSTER_DTYPE array in upstream's final order, members holds indices into `matches`."""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    dists, rects = _side_car(obj_origin_dists, rects)
    pp = _cluster_params(vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh)
    clusters, members, n = _cluster_outputs(len(matches))
    _lib.check(_lib.lib().lmx_cluster_matches(matches.ctypes.data, len(matches), dists.ctypes.data, rects.ctypes.data, len(dists), C.byref(pp),
                                              clusters.ctypes.data, len(clusters), C.byref(n), members.ctypes.data, len(members)))
    return clusters[:n.value].copy(), members


def cluster_matches_scored(matches, match_values, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh=2):
    """lmx_cluster_matches_scored: `cluster_matches` with a cluster's score = the mean of match_values over its members instead of the mean
    similarity (the slot of the reference's depth_normal_diff_calc score; feed it `depth_values(DepthTemplates.diff(...))`).  With
    match_values = matches["similarity"] it equals cluster_matches bit for bit.  Returns (clusters, members)."""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    values = np.ascontiguousarray(match_values, np.float64)
    if values.shape != (len(matches),):
        raise ValueError("match_values must hold one value per match")
    dists, rects = _side_car(obj_origin_dists, rects)
    pp = _cluster_params(vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh)
    clusters, members, n = _cluster_outputs(len(matches))
    _lib.check(_lib.lib().lmx_cluster_matches_scored(matches.ctypes.data, len(matches), values.ctypes.data, dists.ctypes.data, rects.ctypes.data, len(dists),
                                                     C.byref(pp), clusters.ctypes.data, len(clusters), C.byref(n), members.ctypes.data, len(members)))
    return clusters[:n.value].copy(), members


def _class_sidecars(classes):
    """classes: one entry per class index, None (no side-car) or (obj_origin_dists, rects, vote_row_col_step, renderer_radius_min,
    renderer_radius_step, cluster_size_thresh) -> (lmx_class_sidecar array, the arrays it points into)."""
    arr = (_lib.ClassSidecar * max(1, len(classes)))()
    keep = []
    for k, c in enumerate(classes):
        if c is None:
            continue
        d, r = _side_car(c[0], c[1])
        if len(r) != len(d):
            raise ValueError("class %d: one rect per origin distance" % k)
        keep += [d, r]
        arr[k] = _lib.ClassSidecar(d.ctypes.data if len(d) else None, r.ctypes.data if len(d) else None, len(d), _cluster_params(*c[2:]))
    return arr, keep


def cluster_matches_classes(matches, classes, match_values=None):
    """lmx_cluster_matches_classes: the chain of cluster_matches (match_values None) or cluster_matches_scored per class of a bank of
    several classes.  classes[c]: None or (obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step,
    cluster_size_thresh).  -> (clusters, cluster_class, members): class 0's clusters in the chain's order, then class 1's, ...; members
    index `matches`.  Matches of a class without a side-car belong to no cluster; the NMS never crosses classes."""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    values = None
    if match_values is not None:
        values = np.ascontiguousarray(match_values, np.float64)
        if values.shape != (len(matches),):
            raise ValueError("match_values must hold one value per match")
    arr, keep = _class_sidecars(classes)
    clusters, members, n = _cluster_outputs(len(matches))
    cluster_class = np.zeros(len(clusters), np.int32)
    _lib.check(_lib.lib().lmx_cluster_matches_classes(matches.ctypes.data, len(matches), values.ctypes.data if values is not None else None, arr, len(classes),
                                                      clusters.ctypes.data, cluster_class.ctypes.data, len(clusters), C.byref(n), members.ctypes.data,
                                                      len(members)))
    del keep
    return clusters[:n.value].copy(), cluster_class[:n.value].copy(), members


def depth_values(diffs):
    """Per-match values for cluster_matches_scored from DepthTemplates.diff results: minus the mean absolute depth difference in metres,
    -(sum_abs_mm / (n_valid * 1000)).  The reference's getClusterScore (src/rgbdDetector.cpp:576-584) is 1 / exp(mean difference in m) with
    the normal term left out; exp is monotonic, so clusters rank the same.  A match with n_valid == 0 (nothing to compare) gets -inf:
    a cluster that holds one goes to the end."""
    diffs = np.asarray(diffs, DEPTH_DIFF_DTYPE)
    out = np.full(len(diffs), -np.inf)
    ok = diffs["n_valid"] > 0
    out[ok] = -(diffs["sum_abs_mm"][ok].astype(np.float64) / (diffs["n_valid"][ok].astype(np.float64) * 1000.0))
    return out


# lmx_pose_refine_t; status: the LMX_POSE_* values
POSE_REFINE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t_mm", "<f8", (3,)), ("rms_first_mm", "<f8"), ("rms_last_mm", "<f8"), ("n_model", "<i4"),
                              ("n_pairs_first", "<i4"), ("n_pairs_last", "<i4"), ("iterations", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
POSE_NONE, POSE_CONVERGED, POSE_MAX_ITERATIONS, POSE_NO_OVERLAP, POSE_LOST = range(5)


# lmx_pose_verify_t; status: the LMX_VERIFY_* values
POSE_VERIFY_DTYPE = np.dtype([("rate", "<f8"), ("n_model", "<i4"), ("n_tested", "<i4"), ("n_occupied", "<i4"), ("n_scene", "<i4"), ("cells", "<i4"),
                              ("status", "<i4"), ("roi", "<i4", (4,))])
VERIFY_NONE, VERIFY_OK, VERIFY_EMPTY, VERIFY_GRID_TOO_LARGE = range(4)


def keep_verified(records, thresh):
    """The reference's erase rule on DepthTemplates.verify_poses records (lmx_pose_verify_keep): kept iff status is VERIFY_OK and not
    rate < thresh -> bool [len(records)]."""
    records = np.asarray(records, POSE_VERIFY_DTYPE)
    with np.errstate(invalid="ignore"):
        return (records["status"] == VERIFY_OK) & ~(records["rate"] < float(thresh))


def compose_pose(view, record):
    """lmx_pose_compose: the object's pose in the scene camera from the matched template's view (R [3, 3] or 9 values, distance in
    metres) and its DepthTemplates.refine_poses record -> (R_obj [3, 3], t_obj in metres)."""
    R, distance = view
    v = _lib.MeshView((C.c_double * 9)(*np.asarray(R, np.float64).reshape(9)), float(distance))
    rec = np.zeros(1, POSE_REFINE_DTYPE)
    rec[0] = record
    R_obj, t_obj = np.zeros(9), np.zeros(3)
    _lib.check(_lib.lib().lmx_pose_compose(C.byref(v), rec.ctypes.data, R_obj.ctypes.data, t_obj.ctypes.data))
    return R_obj.reshape(3, 3), t_obj


def cluster_leaders(clusters, members, matches):
    """The match each cluster's pose is refined from: per cluster the index (into `matches`) of its member of highest similarity, the
    first in member order on a tie -> int64 [len(clusters)]."""
    members = np.asarray(members)
    out = np.zeros(len(clusters), np.int64)
    for k, c in enumerate(clusters):
        mi = members[int(c["member_begin"]):int(c["member_begin"]) + int(c["member_count"])]
        if len(mi) == 0:
            raise ValueError("cluster %d has no members" % k)
        out[k] = mi[int(np.argmax(np.asarray(matches)["similarity"][mi]))]
    return out


def normal_values(ddiffs, ndiffs):
    """Per-match values for cluster_matches_scored from DepthTemplates.normal_diff results (lmx_match_value): minus (the mean absolute depth
    difference in metres + the mean normal angle in radians); -inf for a match with n_valid == 0 or n_normal == 0.  The mean of it over a
    cluster is the logarithm of the reference's getClusterScore, 1 / exp(depth term) * 1 / exp(normal term)."""
    ddiffs = np.asarray(ddiffs, DEPTH_DIFF_DTYPE)
    ndiffs = np.asarray(ndiffs, NORMAL_DIFF_DTYPE)
    if ddiffs.shape != ndiffs.shape:
        raise ValueError("one depth diff and one normal diff per match")
    out = np.full(len(ddiffs), -np.inf)
    ok = (ddiffs["n_valid"] > 0) & (ndiffs["n_normal"] > 0)
    out[ok] = -(ddiffs["sum_abs_mm"][ok].astype(np.float64) / (ddiffs["n_valid"][ok].astype(np.float64) * 1000.0)
                + ndiffs["sum_angle_urad"][ok].astype(np.float64) / (ndiffs["n_normal"][ok].astype(np.float64) * 1e6))
    return out


def normal_angle_table():
    """lmx_normal_angle_table: uint32 [16385], half chord in 1 / 16384 -> angle in microradians."""
    out = np.zeros(16385, np.uint32)
    _lib.check(_lib.lib().lmx_normal_angle_table(out.ctypes.data))
    return out


def _depth_images(depth_frames):
    """A uint16 [H, W] array or a list of them -> (the list, its lmx_image descriptors)."""
    if isinstance(depth_frames, np.ndarray) and depth_frames.ndim == 2:
        depth_frames = [depth_frames]
    frames = list(depth_frames)
    for d in frames:
        if d.dtype != np.uint16 or d.ndim != 2 or d.strides[1] != 2:
            raise TypeError("depth frames must be uint16 HxW with contiguous rows (the row stride may be larger)")
    return frames, (_lib.Image * max(1, len(frames)))(*[_lib.Image(d.ctypes.data, d.shape[0], d.shape[1], 1, 2, d.strides[0]) for d in frames])


def _frame_offsets(offsets, n_frames, n_matches):
    """Where each frame's matches begin in a list of all frames' back to back (default: one frame holding all) -> size_t [n_frames + 1]."""
    if offsets is None:
        if n_frames != 1:
            raise ValueError("offsets are needed with more than one frame")
        offsets = [0, n_matches]
    if len(offsets) != n_frames + 1 or int(offsets[-1]) != n_matches:
        raise ValueError("offsets must have one entry per frame plus one and end at len(matches)")
    return (C.c_size_t * len(offsets))(*[int(v) for v in offsets])


# ---- the array fields of a chain descriptor (PoseChainDesc, RoughChainDesc): eight of input, and the outputs a result class's NAMES name ----
_CHAIN_HOST_DTYPES = {"chain_header": np.uint32, "leaders": np.int32, "rough": ROUGH_POSE_DTYPE, "member_group": np.int32, "poses": POSE_REFINE_DTYPE,
                      "checks": POSE_VERIFY_DTYPE, "keep": np.uint8}


def _chain_room(exported, out):
    """What a chain call needs of the export it reads and of the `out` it is to write again (None: a fresh one) -> the export's caps."""
    if getattr(exported, "clusters", None) is None or exported.members is None:
        raise ValueError("exported holds no clusters (export_matches(clusters=True) or export_clusters)")
    if exported.caps[1] < 1:
        raise ValueError("the export has no room for clusters")
    if out is not None:
        out._fits(exported.caps)
    return exported.caps


def _chain_inputs(d, exported):
    """The eight input fields of d from an export's tensors and capacities."""
    b, caps = exported._backing, exported.caps
    d.header, d.frame_info, d.matches, d.cap_matches = b["header"].data_ptr(), b["frame_info"].data_ptr(), b["matches"].data_ptr(), caps[0]
    d.clusters, d.cap_clusters, d.members, d.cap_members = b["clusters"].data_ptr(), caps[1], b["members"].data_ptr(), caps[2]


def _chain_inputs_host(d, lists, cap_clusters=None):
    """The same from lists = (header, frame_info, matches, clusters, members) in host memory, whose lengths are the capacities; cap_clusters
    may state a smaller one.  -> the lists as the arrays d points to: uint32 [16], int32 [F, 8], MATCH_DTYPE, CLUSTER_DTYPE, int32."""
    header, frame_info, matches, clusters, members = lists
    header = np.ascontiguousarray(header).astype(np.uint32).reshape(16)
    frame_info = np.ascontiguousarray(frame_info, np.int32).reshape(-1, 8)
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    clusters = np.ascontiguousarray(clusters, CLUSTER_DTYPE)
    members = np.ascontiguousarray(members, np.int32)
    d.header, d.frame_info, d.matches, d.cap_matches = header.ctypes.data, frame_info.ctypes.data, matches.ctypes.data, len(matches)
    d.clusters, d.cap_clusters, d.members, d.cap_members = clusters.ctypes.data, len(clusters) if cap_clusters is None else int(cap_clusters), members.ctypes.data, len(members)
    if d.cap_clusters > len(clusters):
        raise ValueError("cap_clusters exceeds len(clusters)")
    return header, frame_info, matches, clusters, members


def _chain_outputs_host(names, n_clusters, n_members, fill):
    """The arrays a debug chain hook writes, name -> array: chain_header zeroed, the others -- one entry per cluster, member_group per
    member (at least one) -- holding the byte `fill`."""
    out = {k: np.zeros(POSE_CHAIN_HEADER_WORDS if k == "chain_header" else max(n_members, 1) if k == "member_group" else n_clusters, _CHAIN_HOST_DTYPES[k])
           for k in names}
    for k in names:
        if k != "chain_header":
            out[k].view(np.uint8)[:] = fill
    return out


def _chain_outputs(d, names, address):
    """The output fields `names` of d from a mapping name -> address."""
    for k in names:
        setattr(d, k, address[k])


class DepthTemplates:
    """Device-resident depth renders of a bank's templates, cropped to their silhouette boxes (lmx_depth_templates), and the depth check
    of matches against them (lmx_depth_diff_matches): the depth half of the reference's depth_normal_diff_calc
    (src/rgbdDetector.cpp:147-282) without the per-match re-render."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    @classmethod
    def from_mesh(cls, triangles, views, width, height, fx, fy, cx=None, cy=None, light=MESH_LIGHT, device=0):
        """One template per (R, distance) of `views`, in order: for a bank from NativeBank.train_mesh, zip(last_side_car["R"],
        last_side_car["T"][:, 2]).  Any iterable of pairs."""
        views = list(views)
        tri, cam, packed = _mesh_args(triangles, views, width, height, fx, fy, cx, cy, light)
        h = C.c_void_p()
        _lib.check(_lib.lib().lmx_depth_templates_from_mesh(device, tri.ctypes.data, tri.shape[0], C.byref(cam), packed.ctypes.data_as(C.POINTER(_lib.MeshView)),
                                                            len(views), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_crops(cls, crops, device=0):
        """Ready-made crops: a list of uint16 [h, w] arrays (0 = not on the object); empty arrays are allowed."""
        keep = []
        for c in crops:
            c = np.ascontiguousarray(c, np.uint16)
            if c.ndim != 2:
                raise TypeError("a crop must be a uint16 [h, w] array")
            keep.append(c)
        n = len(keep)
        ptrs = (C.c_void_p * max(1, n))(*[c.ctypes.data if c.size else None for c in keep])
        sizes = (C.c_int32 * max(2, 2 * n))(*[v for c in keep for v in (c.shape[1], c.shape[0])])
        h = C.c_void_p()
        _lib.check(_lib.lib().lmx_depth_templates_from_crops(device, ptrs, sizes, n, C.byref(h)))
        return cls(h.value)

    def __len__(self):
        return int(_lib.lib().lmx_depth_templates_count(self.h))

    def rect(self, i):
        """(x, y, w, h): from_mesh: the silhouette box in the rendered view; from_crops: (0, 0, w, h)."""
        r = (C.c_int32 * 4)()
        _lib.check(_lib.lib().lmx_depth_templates_rect(self.h, int(i), r))
        return tuple(r)

    def crop(self, i):
        """Template i's crop, read back from the device: uint16 [h, w]."""
        _, _, w, h = self.rect(i)
        out = np.zeros((h, w), np.uint16)
        _lib.check(_lib.lib().lmx_depth_templates_get(self.h, int(i), out.ctypes.data))
        return out

    @property
    def device_bytes(self):
        return int(_lib.lib().lmx_depth_templates_device_bytes(self.h))

    def diff(self, depth_frames, matches, offsets=None, class_index=-1):
        """depth_frames: a uint16 [H, W] array or a list of them (all of one size; rows may be strided); matches: MATCH_DTYPE records of
        all frames back to back, frame f's at offsets[f]:offsets[f + 1] (default: one frame holding all).  -> DEPTH_DIFF_DTYPE array, one
        record per match; with class_index >= 0 the matches of other classes get zeros."""
        frames, imgs = _depth_images(depth_frames)
        matches = np.ascontiguousarray(matches, MATCH_DTYPE)
        offs = _frame_offsets(offsets, len(frames), len(matches))
        out = np.zeros(len(matches), DEPTH_DIFF_DTYPE)
        _lib.check(_lib.lib().lmx_depth_diff_matches(self.h, imgs, len(frames), matches.ctypes.data, offs, int(class_index), out.ctypes.data))
        return out

    def enable_normals(self, fx, fy, difference_threshold=50, distance_threshold=2000):
        """Compute and keep the normals of every crop (lmx_depth_templates_enable_normals): needed before normals(), normal_diff() and
        Detector.collect_clusters_depth_normal.  fx, fy: the focal lengths of the camera whose depth frames are checked."""
        p = _lib.NormalParams(float(fx), float(fy), int(difference_threshold), int(distance_threshold))
        _lib.check(_lib.lib().lmx_depth_templates_enable_normals(self.h, C.byref(p)))

    def normals(self, i):
        """Template i's normals, read back from the device: int16 [h, w, 4] = (qx, qy, qz, valid), a unit normal times 16384."""
        _, _, w, h = self.rect(i)
        out = np.zeros((h, w, 4), np.int16)
        _lib.check(_lib.lib().lmx_depth_templates_get_normals(self.h, int(i), out.ctypes.data))
        return out

    def normal_diff(self, depth_frames, matches, offsets=None, class_index=-1):
        """diff() with both terms in one pass (lmx_normal_diff_matches) -> (DEPTH_DIFF_DTYPE array, NORMAL_DIFF_DTYPE array), one record
        per match each; the first equals diff()'s result."""
        frames, imgs = _depth_images(depth_frames)
        matches = np.ascontiguousarray(matches, MATCH_DTYPE)
        offs = _frame_offsets(offsets, len(frames), len(matches))
        dd = np.zeros(len(matches), DEPTH_DIFF_DTYPE)
        nd = np.zeros(len(matches), NORMAL_DIFF_DTYPE)
        _lib.check(_lib.lib().lmx_normal_diff_matches(self.h, imgs, len(frames), matches.ctypes.data, offs, int(class_index), dd.ctypes.data, nd.ctypes.data))
        return dd, nd

    def _pose_frames(self, matches, depth_frames, offsets):
        """The frame arguments of refine_poses / verify_poses -> (frames to keep alive, lmx_image array or None, n_frames, size_t offsets)."""
        if depth_frames is not None:
            frames, imgs = _depth_images(depth_frames)
            n_frames = len(frames)
        else:
            frames, imgs = None, None
            n_frames = len(offsets) - 1 if offsets is not None else 1
        return frames, imgs, n_frames, _frame_offsets(offsets, n_frames, len(matches))

    def _pose_rects(self, rects):
        keep = np.ascontiguousarray(rects, np.int32).reshape(-1, 4) if rects is not None else None
        if keep is not None and len(keep) != len(self):
            raise ValueError("rects must hold one (x, y, w, h) per template")
        return keep

    def _pose_params(self, model_camera, scene_camera, max_dist_mm, max_iterations, min_pairs, search_radius, eps_rot_rad, eps_trans_mm, rects):
        if model_camera is None or scene_camera is None:
            raise ValueError("model_camera and scene_camera are (fx, fy, cx, cy)")
        keep = self._pose_rects(rects)
        p = _lib.PoseRefineParams(C.sizeof(_lib.PoseRefineParams), *[float(v) for v in tuple(model_camera) + tuple(scene_camera)], float(max_dist_mm),
                                  float(eps_rot_rad), float(eps_trans_mm), int(max_iterations), int(min_pairs), int(search_radius),
                                  keep.ctypes.data if keep is not None else None)
        return p, keep

    @staticmethod
    def _verify_params(model_camera, scene_camera, voxel_mm, roi_margin, keep):
        """keep: what _pose_rects returned."""
        return _lib.PoseVerifyParams(C.sizeof(_lib.PoseVerifyParams), *[float(v) for v in tuple(model_camera) + tuple(scene_camera)], float(voxel_mm), int(roi_margin),
                                     keep.ctypes.data if keep is not None else None)

    STAGE_FIELDS = ("max_dist_mm", "eps_rot_rad", "eps_trans_mm", "max_iterations", "search_radius", "stride")

    def set_refine_schedule(self, stages):
        """The refinement schedule of this object (lmx_depth_templates_set_refine_schedule): a list of 1 to 4 dicts with the keys
        STAGE_FIELDS -- a stage's own correspondence distance, stopping rule, window and a stride in (1, 2, 4, 8) that thins the model
        pixels to a lattice; each stage starts from the pose the one before it left.  None or []: no schedule.  While one is set,
        refine_poses, debug_pose_refine_sums and the pose chains refine by it and take only the cameras, min_pairs and rects from their
        own parameters.  Work already queued keeps the schedule it was queued under."""
        stages = list(stages) if stages is not None else []
        for st in stages:
            if set(st) != set(self.STAGE_FIELDS):
                raise ValueError("a stage is a dict with the keys %s" % (self.STAGE_FIELDS,))
        arr = (_lib.PoseRefineStage * max(len(stages), 1))()
        for k, st in enumerate(stages):
            arr[k] = _lib.PoseRefineStage(float(st["max_dist_mm"]), float(st["eps_rot_rad"]), float(st["eps_trans_mm"]), int(st["max_iterations"]),
                                          int(st["search_radius"]), int(st["stride"]), 0)
        _lib.check(_lib.lib().lmx_depth_templates_set_refine_schedule(self.h, arr if stages else None, len(stages)))

    @property
    def refine_schedule(self):
        """The schedule in force (lmx_depth_templates_get_refine_schedule): a list of dicts as set_refine_schedule takes them, [] for none."""
        arr = (_lib.PoseRefineStage * _lib.LMX_POSE_MAX_STAGES)()
        n = C.c_int32(0)
        _lib.check(_lib.lib().lmx_depth_templates_get_refine_schedule(self.h, arr, C.byref(n)))
        return [{k: getattr(arr[i], k) for k in self.STAGE_FIELDS} for i in range(n.value)]

    def set_refine_plane(self, point_shift):
        """The stages' point_shift (lmx_depth_templates_set_refine_plane): a list of up to 4 integers, entry s for stage s of the schedule in
        force (a call without one is stage 0).  -1: the point-to-point stage; k in 0..20: point-to-plane against the scene's stored normals
        (enable_normals first), the point term weighted 2**-k -- meant for few iterations.  None or []: clears the setting."""
        shifts = [int(v) for v in point_shift] if point_shift is not None else []
        arr = (C.c_int32 * max(len(shifts), 1))(*shifts)
        _lib.check(_lib.lib().lmx_depth_templates_set_refine_plane(self.h, arr if shifts else None, len(shifts)))

    def get_refine_plane(self):
        """The point_shift list in force (lmx_depth_templates_get_refine_plane), [] for none."""
        arr = (C.c_int32 * _lib.LMX_POSE_MAX_STAGES)()
        n = C.c_int32(0)
        _lib.check(_lib.lib().lmx_depth_templates_get_refine_plane(self.h, arr, C.byref(n)))
        return [int(arr[i]) for i in range(n.value)]

    def refine_poses(self, matches, depth_frames=None, offsets=None, class_index=-1, model_camera=None, scene_camera=None, max_dist_mm=10.0,
                     max_iterations=20, min_pairs=16, search_radius=1, eps_rot_rad=1e-5, eps_trans_mm=1e-3, rects=None):
        """A rigid transform per match (lmx_pose_refine_matches; the reference's icpPoseRefine stage) -> POSE_REFINE_DTYPE array: R, t_mm map
        a point of the matched template's view (model camera frame, mm) into the scene camera frame.  matches / offsets / class_index as
        diff(); depth_frames None: the scene upload_scene / upload_scene_device left in the object, and offsets must then have one entry
        per frame of it plus one.  model_camera / scene_camera: (fx, fy, cx, cy) of the camera the crops were rendered with and of the
        depth frames.  rects: [n, 4] int32 instead of the object's own silhouette boxes (needed for an object made from_crops)."""
        matches = np.ascontiguousarray(matches, MATCH_DTYPE)
        frames, imgs, n_frames, offs = self._pose_frames(matches, depth_frames, offsets)
        p, keep = self._pose_params(model_camera, scene_camera, max_dist_mm, max_iterations, min_pairs, search_radius, eps_rot_rad, eps_trans_mm, rects)
        out = np.zeros(len(matches), POSE_REFINE_DTYPE)
        _lib.check(_lib.lib().lmx_pose_refine_matches(self.h, imgs, n_frames, matches.ctypes.data, offs, int(class_index), C.byref(p), out.ctypes.data))
        del keep, frames
        return out

    def verify_poses(self, matches, poses, depth_frames=None, offsets=None, class_index=-1, model_camera=None, scene_camera=None, voxel_mm=4.0, roi_margin=8,
                     rects=None):
        """The voxel-occupancy check of refined poses (lmx_pose_verify_matches; the reference's hypothesisVerification stage) ->
        POSE_VERIFY_DTYPE array.  poses: what refine_poses returned for the same matches; the other arguments as refine_poses.  voxel_mm:
        the voxel's side; roi_margin: how many pixels around the posed model's projection the scene is looked at."""
        matches = np.ascontiguousarray(matches, MATCH_DTYPE)
        poses = np.ascontiguousarray(poses, POSE_REFINE_DTYPE)
        if len(poses) != len(matches):
            raise ValueError("poses must hold one record per match")
        if model_camera is None or scene_camera is None:
            raise ValueError("model_camera and scene_camera are (fx, fy, cx, cy)")
        frames, imgs, n_frames, offs = self._pose_frames(matches, depth_frames, offsets)
        keep = self._pose_rects(rects)
        p = self._verify_params(model_camera, scene_camera, voxel_mm, roi_margin, keep)
        out = np.zeros(len(matches), POSE_VERIFY_DTYPE)
        _lib.check(_lib.lib().lmx_pose_verify_matches(self.h, imgs, n_frames, matches.ctypes.data, offs, int(class_index), poses.ctypes.data, C.byref(p),
                                                      out.ctypes.data))
        del keep, frames
        return out

    def _pose_chain_desc(self, n_frames, keep_thresh, class_index, class_base, model_camera, scene_camera, max_dist_mm, max_iterations, min_pairs, search_radius,
                         eps_rot_rad, eps_trans_mm, voxel_mm, roi_margin, rects):
        """The parameters of pose_chain / debug_pose_chain -> (PoseChainDesc without its arrays, what it points to)."""
        pr, keep = self._pose_params(model_camera, scene_camera, max_dist_mm, max_iterations, min_pairs, search_radius, eps_rot_rad, eps_trans_mm, rects)
        pv = self._verify_params(model_camera, scene_camera, voxel_mm, roi_margin, keep)
        base = _class_base(class_base) if class_base is not None else None
        d = _lib.PoseChainDesc()
        d.struct_size, d.n_frames, d.class_index, d.n_classes = C.sizeof(_lib.PoseChainDesc), int(n_frames), int(class_index), len(base) - 1 if base is not None else 0
        d.class_base = base.ctypes.data if base is not None else None
        d.refine, d.verify, d.keep_thresh = C.pointer(pr), C.pointer(pv), float(keep_thresh)
        return d, (pr, pv, keep, base)

    def pose_chain(self, exported, keep_thresh, model_camera=None, scene_camera=None, max_dist_mm=10.0, max_iterations=20, min_pairs=16, search_radius=1,
                   eps_rot_rad=1e-5, eps_trans_mm=1e-3, voxel_mm=4.0, roi_margin=8, rects=None, class_index=-1, class_base=None, stream=None, out=None):
        """Both pose stages on the clusters an export left on the GPU (lmx_pose_chain_on) -> ExportedPoses: per exported cluster the
        leader of cluster_leaders, its refine_poses record, its verify_poses record and the keep_verified decision, equal in every byte to
        those four run on to_host()'s lists against the same resident scene -- with no host wait in between.  exported: an
        ExportedMatches (clusters=True) or an ExportedClusters; the scene: what upload_scene / upload_scene_device left in this object, of
        exported.n_frames frames.  keep_thresh: the reference's 0.3 (carmine) or 0.2 (ensenso).  The keywords of refine_poses and
        verify_poses; class_base: the cumulative template counts of the classes joined in this object (append), a match's template_id is
        then rebased by its class.  stream: default exported.stream.  out: an ExportedPoses of an earlier call with room for the export's
        cluster capacity, written again in place of fresh tensors."""
        caps = _chain_room(exported, out)
        if model_camera is None or scene_camera is None:
            raise ValueError("model_camera and scene_camera are (fx, fy, cx, cy)")
        device = exported.header.device.index
        stream = _torch_stream(stream, exported.stream, device)
        if out is None:
            out = ExportedPoses(caps[1], stream, device)
        out.stream = stream
        d, alive = self._pose_chain_desc(exported.n_frames, keep_thresh, class_index, class_base, model_camera, scene_camera, max_dist_mm, max_iterations, min_pairs,
                                         search_radius, eps_rot_rad, eps_trans_mm, voxel_mm, roi_margin, rects)
        _chain_inputs(d, exported)
        _chain_outputs(d, out.NAMES, {k: v.data_ptr() for k, v in out._backing.items()})
        _lib.check(_lib.lib().lmx_pose_chain_on(self.h, C.byref(d), int(stream.cuda_stream)))
        del alive
        return out

    def debug_pose_chain(self, header, frame_info, matches, clusters, members, keep_thresh, cap_clusters=None, fill=0, class_index=-1, class_base=None,
                         model_camera=None, scene_camera=None, max_dist_mm=10.0, max_iterations=20, min_pairs=16, search_radius=1, eps_rot_rad=1e-5,
                         eps_trans_mm=1e-3, voxel_mm=4.0, roi_margin=8, rects=None):
        """Test hook (lmx_debug_pose_chain): pose_chain's two kernels on lists in host memory (header int32 / uint32 [16], frame_info int32
        [F, 8], matches MATCH_DTYPE, clusters CLUSTER_DTYPE, members int32; their lengths are the capacities, cap_clusters may state a
        smaller one) against the resident scene -> (chain_header uint32 [8], leaders int32, poses POSE_REFINE_DTYPE, checks
        POSE_VERIFY_DTYPE, keep uint8), each [len(clusters)] and holding the byte `fill` wherever the kernels wrote nothing."""
        d, alive = self._pose_chain_desc(0, keep_thresh, class_index, class_base, model_camera, scene_camera, max_dist_mm, max_iterations, min_pairs,
                                         search_radius, eps_rot_rad, eps_trans_mm, voxel_mm, roi_margin, rects)
        lists = _chain_inputs_host(d, (header, frame_info, matches, clusters, members), cap_clusters)
        d.n_frames = len(lists[1])
        out = _chain_outputs_host(ExportedPoses.NAMES, len(lists[3]), len(lists[4]), fill)
        _chain_outputs(d, ExportedPoses.NAMES, {k: a.ctypes.data for k, a in out.items()})
        _lib.check(_lib.lib().lmx_debug_pose_chain(self.h, C.byref(d)))
        del alive, lists
        return tuple(out[k] for k in ExportedPoses.NAMES)

    def _rough_chain_desc(self, model, n_frames, keep_thresh, threshold_deg, trace_min, class_index, model_camera, scene_camera, max_dist_mm, max_iterations,
                          min_pairs, search_radius, eps_rot_rad, eps_trans_mm, voxel_mm, roi_margin):
        """The parameters of rough_pose_chain / debug_rough_pose_chain -> (RoughChainDesc without its arrays, what it points to)."""
        if model_camera is None:
            model_camera = model.camera
        if scene_camera is None:
            raise ValueError("scene_camera is (fx, fy, cx, cy)")
        pr, _ = self._pose_params(model_camera, scene_camera, max_dist_mm, max_iterations, min_pairs, search_radius, eps_rot_rad, eps_trans_mm, None)
        pv = self._verify_params(model_camera, scene_camera, voxel_mm, roi_margin, None)
        d = _lib.RoughChainDesc()
        d.struct_size, d.n_frames, d.class_index = C.sizeof(_lib.RoughChainDesc), int(n_frames), int(class_index)
        d.refine, d.verify, d.keep_thresh = C.pointer(pr), C.pointer(pv), float(keep_thresh)
        d.trace_min = float(trace_min) if trace_min is not None else rough_trace_min(threshold_deg)
        return d, (pr, pv)

    def rough_pose_chain(self, exported, model, keep_thresh, threshold_deg=10.0, scene_camera=None, model_camera=None, max_dist_mm=10.0, max_iterations=20, min_pairs=16,
                         search_radius=1, eps_rot_rad=1e-5, eps_trans_mm=1e-3, voxel_mm=4.0, roi_margin=8, class_index=-1, trace_min=None, stream=None, out=None):
        """The reference's getRoughPoseByClustering in front of both pose stages, on the clusters an export left on the GPU
        (lmx_rough_pose_chain_on) -> ExportedRoughPoses: per exported cluster the mean view of its largest orientation group (views closer
        than threshold_deg to the member that opened the group), the mesh of `model` (a RoughModel whose views are indexed by the matches'
        template_id) rendered again at that view, that render refined and verified against the resident scene at the mean match
        position, and the keep decision -- with no host wait in between.  model_camera: default the model's.  trace_min: in place of
        threshold_deg, the bound itself.  The other keywords as pose_chain; rects are the rendered ones."""
        caps = _chain_room(exported, out)
        device = exported.header.device.index
        stream = _torch_stream(stream, exported.stream, device)
        if out is None:
            out = ExportedRoughPoses(caps[1], caps[2], stream, device)
        out.stream = stream
        d, alive = self._rough_chain_desc(model, exported.n_frames, keep_thresh, threshold_deg, trace_min, class_index, model_camera, scene_camera, max_dist_mm,
                                          max_iterations, min_pairs, search_radius, eps_rot_rad, eps_trans_mm, voxel_mm, roi_margin)
        _chain_inputs(d, exported)
        _chain_outputs(d, out.NAMES, {k: v.data_ptr() for k, v in out._backing.items()})
        _lib.check(_lib.lib().lmx_rough_pose_chain_on(self.h, model.h, C.byref(d), int(stream.cuda_stream)))
        del alive
        return out

    def debug_rough_pose_chain(self, model, header, frame_info, matches, clusters, members, keep_thresh, threshold_deg=10.0, cap_clusters=None, fill=0, class_index=-1,
                               trace_min=None, scene_camera=None, model_camera=None, max_dist_mm=10.0, max_iterations=20, min_pairs=16, search_radius=1,
                               eps_rot_rad=1e-5, eps_trans_mm=1e-3, voxel_mm=4.0, roi_margin=8):
        """Test hook (lmx_debug_rough_pose_chain): rough_pose_chain's kernels on lists in host memory, as debug_pose_chain takes them ->
        (chain_header uint32 [8], rough ROUGH_POSE_DTYPE, member_group int32 [len(members)], poses, checks, keep), holding the byte `fill`
        wherever the kernels wrote nothing."""
        d, alive = self._rough_chain_desc(model, 0, keep_thresh, threshold_deg, trace_min, class_index, model_camera, scene_camera, max_dist_mm,
                                          max_iterations, min_pairs, search_radius, eps_rot_rad, eps_trans_mm, voxel_mm, roi_margin)
        lists = _chain_inputs_host(d, (header, frame_info, matches, clusters, members), cap_clusters)
        d.n_frames = len(lists[1])
        out = _chain_outputs_host(ExportedRoughPoses.NAMES, len(lists[3]), len(lists[4]), fill)
        _chain_outputs(d, ExportedRoughPoses.NAMES, {k: a.ctypes.data for k, a in out.items()})
        _lib.check(_lib.lib().lmx_debug_rough_pose_chain(self.h, model.h, C.byref(d)))
        out["member_group"] = out["member_group"][:len(lists[4])]
        del alive, lists
        return tuple(out[k] for k in ExportedRoughPoses.NAMES)

    def debug_pose_refine_sums(self, depth_frame, match, **params):
        """Test hook (lmx_debug_pose_refine_sums): one match against one host frame -> (its POSE_REFINE_DTYPE record, int64
        [max_iterations + 1, 17]: the integer sums of every pass the device ran; under a schedule one row per pass of its stages, in the
        order they ran, [sum of max_iterations + 1, 17])."""
        frames, imgs = _depth_images(depth_frame)
        m = np.ascontiguousarray(match, MATCH_DTYPE).reshape(1)
        args = dict(max_dist_mm=10.0, max_iterations=20, min_pairs=16, search_radius=1, eps_rot_rad=1e-5, eps_trans_mm=1e-3, rects=None)
        args.update(params)
        p, keep = self._pose_params(**args)
        out = np.zeros(1, POSE_REFINE_DTYPE)
        sched = self.refine_schedule
        sums = np.zeros(((sum(st["max_iterations"] for st in sched) if sched else int(args["max_iterations"])) + 1, 17), np.int64)
        _lib.check(_lib.lib().lmx_debug_pose_refine_sums(self.h, imgs, m.ctypes.data, C.byref(p), out.ctypes.data, sums.ctypes.data))
        del keep, frames
        return out[0], sums

    def debug_pose_refine_plane_sums(self, depth_frame, match, **params):
        """Test hook (lmx_debug_pose_refine_plane_sums): debug_pose_refine_sums and, row for row, the 29 plane sums of every pass ->
        (record, int64 [passes, 17], int64 [passes, 29]); the plane rows of point-to-point passes are zeros."""
        frames, imgs = _depth_images(depth_frame)
        m = np.ascontiguousarray(match, MATCH_DTYPE).reshape(1)
        args = dict(max_dist_mm=10.0, max_iterations=20, min_pairs=16, search_radius=1, eps_rot_rad=1e-5, eps_trans_mm=1e-3, rects=None)
        args.update(params)
        p, keep = self._pose_params(**args)
        out = np.zeros(1, POSE_REFINE_DTYPE)
        sched = self.refine_schedule
        rows = (sum(st["max_iterations"] for st in sched) if sched else int(args["max_iterations"])) + 1
        sums, plane = np.zeros((rows, 17), np.int64), np.zeros((rows, 29), np.int64)
        _lib.check(_lib.lib().lmx_debug_pose_refine_plane_sums(self.h, imgs, m.ctypes.data, C.byref(p), out.ctypes.data, sums.ctypes.data, plane.ctypes.data))
        del keep, frames
        return out[0], sums, plane

    # Labels of the library's profiling brackets (its PK_* enum, in that order), not symbol names: "k_verify_diff_records", "k_verify_diff"
    # and "k_depth_diff_records" are the record walk with both terms, the job walk with both terms and the depth-only record walk (all
    # instantiations of k_walk, csrc/lmx_verify.hip); the depth-only job walk has no bracket.
    KERNELS = ("k_normal_map_frames", "k_verify_diff_records", "k_verify_diff", "k_depth_diff_records", "k_walk_records_dev", "k_pose_refine", "k_pose_verify",
               "k_pose_refine_clusters", "k_pose_verify_clusters", "k_scene_filter_score", "k_scene_filter_apply")

    def set_profiling(self, on=True):
        """Time the object's per-call kernels with device events (lmx_depth_templates_set_profiling); switching it on clears the sums."""
        _lib.check(_lib.lib().lmx_depth_templates_set_profiling(self.h, int(bool(on))))

    def kernel_times(self):
        """-> {kernel name: (total ms, launches)} since profiling was switched on; waits for the launches in flight."""
        out = {}
        for k, name in enumerate(self.KERNELS):
            ms, n = C.c_double(), C.c_int64()
            _lib.check(_lib.lib().lmx_depth_templates_kernel_time(self.h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def debug_scene_normals(self, frame):
        """Test hook (lmx_debug_scene_normals): the normals of frame `frame` of the uploaded scene, int16 [H, W, 4]."""
        if getattr(self, "_scene_shape", None) is None:
            raise ValueError("no scene uploaded through this object")
        out = np.zeros(self._scene_shape + (4,), np.int16)
        _lib.check(_lib.lib().lmx_debug_scene_normals(self.h, int(frame), out.ctypes.data))
        return out

    SCENE_FILTER_INFO_FIELDS = ("n_valid", "n_sparse", "n_scored", "n_removed", "sum_q", "sum_qq", "threshold")

    def set_scene_filter(self, radius=3, k=15, stddev_mul=1.0, camera=None):
        """The depth outlier filter of the scene ahead of the pose stages (lmx_depth_templates_set_scene_filter; the reference's
        statisticalOutlierRemoval).  While it is set, refine_poses, verify_poses, pose_chain, rough_pose_chain and their debug hooks read
        a copy of the scene -- uploaded or passed as depth_frames -- in which every outlier pixel is 0; the cluster scores keep the raw
        scene.  camera: (fx, fy, cx, cy) of the depth frames; it is not compared with a later call's scene_camera.  radius 1..7: the
        window; k: how many nearest window neighbours a pixel's score averages (fewer within 1024 mm: the pixel goes); stddev_mul in
        [0, 16]: pixels scoring above the frame's mean + stddev_mul standard deviations go.  set_scene_filter(None) turns it off."""
        if radius is None:
            if (k, stddev_mul, camera) != (15, 1.0, None):
                raise ValueError("set_scene_filter(None) turns the filter off and takes no other argument")
            _lib.check(_lib.lib().lmx_depth_templates_set_scene_filter(self.h, None))
            return
        if camera is None:
            raise ValueError("camera is (fx, fy, cx, cy) of the depth frames")
        p = _lib.SceneFilterParams()
        _lib.check(_lib.lib().lmx_scene_filter_defaults(C.byref(p)))
        p.radius, p.k, p.stddev_mul = int(radius), int(k), float(stddev_mul)
        p.fx, p.fy, p.cx, p.cy = [float(v) for v in camera]
        _lib.check(_lib.lib().lmx_depth_templates_set_scene_filter(self.h, C.byref(p)))

    def debug_scene_filtered(self, frame):
        """Test hook (lmx_debug_scene_filtered): the filtered copy of frame `frame` of the uploaded scene -> (uint16 [H, W], the frame's
        record as a dict with the keys SCENE_FILTER_INFO_FIELDS)."""
        if getattr(self, "_scene_shape", None) is None:
            raise ValueError("no scene uploaded through this object")
        out = np.zeros(self._scene_shape, np.uint16)
        info = _lib.SceneFilterInfo()
        _lib.check(_lib.lib().lmx_debug_scene_filtered(self.h, int(frame), out.ctypes.data, C.byref(info)))
        return out, {k: getattr(info, k) for k in self.SCENE_FILTER_INFO_FIELDS}

    def debug_walk_records(self, records, header_count, n_candidates, cap, grid_workgroups, class_index=-1, class_base=None, normals=False,
                           fill=None):
        """Test hook (lmx_debug_depth_walk_records): the persistent walk of Detector.export_clusters on RAW_MATCH_DTYPE `records` behind a
        header {n_candidates, header_count}, list capacity `cap`, against the uploaded scene -> (DEPTH_DIFF_DTYPE [n], NORMAL_DIFF_DTYPE [n]
        or None).  fill: the byte every output entry holds before the kernel runs (default 0)."""
        records = np.ascontiguousarray(records, RAW_MATCH_DTYPE)
        n = len(records)
        d = np.zeros(max(n, 1), DEPTH_DIFF_DTYPE)
        nd = np.zeros(max(n, 1), NORMAL_DIFF_DTYPE) if normals else None
        if fill is not None:
            d.view(np.uint8)[:] = fill
            if nd is not None:
                nd.view(np.uint8)[:] = fill
        base = np.ascontiguousarray(class_base, np.int32).reshape(-1) if class_base is not None else None
        _lib.check(_lib.lib().lmx_debug_depth_walk_records(self.h, records.ctypes.data if n else None, n, int(header_count), int(n_candidates), int(cap),
                                                           int(grid_workgroups), int(class_index), base.ctypes.data if base is not None else None,
                                                           len(base) - 1 if base is not None else 0, d.ctypes.data, nd.ctypes.data if nd is not None else None))
        return d[:n], (nd[:n] if nd is not None else None)

    def debug_walk_grid(self, workgroups):
        """Measurement hook (lmx_debug_depth_walk_grid): the grid of the persistent walk from now on; 0 = the default."""
        _lib.check(_lib.lib().lmx_debug_depth_walk_grid(self.h, int(workgroups)))

    def upload_scene(self, depth_frames):
        """The scene of the next Detector.collect_clusters_depth (lmx_depth_templates_upload_scene): a uint16 [H, W] array or a list of
        them, one per frame of the enqueue.  Returns without waiting for the transfer: call it right after Detector.enqueue.  A later
        upload_scene replaces the scene; diff() forgets it whenever it has a match to check."""
        frames, imgs = _depth_images(depth_frames)
        _lib.check(_lib.lib().lmx_depth_templates_upload_scene(self.h, imgs, len(frames)))
        self._scene_shape = tuple(frames[0].shape)

    def upload_scene_device(self, depth_frames, stream=None):
        """upload_scene for depth frames in this object's GPU memory (lmx_depth_templates_upload_scene_device): a uint16 / int16 [H, W]
        tensor (or object with __cuda_array_interface__) or a list of them.  `stream` as in Detector.upload_device."""
        frames = list(depth_frames) if isinstance(depth_frames, (list, tuple)) else [depth_frames]
        imgs, keep = device_images([[d] for d in frames])
        if any(im.elem_size != 2 or im.channels != 1 for im in imgs):
            raise ValueError("depth frames must be uint16 / int16 HxW")
        _lib.check(_lib.lib().lmx_depth_templates_upload_scene_device(self.h, imgs, len(frames), _device_stream(keep, stream)))
        self._scene_shape = (int(imgs[0].rows), int(imgs[0].cols))

    def append(self, other):
        """Move `other`'s templates behind this object's (lmx_depth_templates_append): other's template i becomes template len(self) + i,
        `other` is left empty.  For the per-class chain: the classes' objects joined in class order, class_base their cumulative counts.
        An uploaded scene is forgotten."""
        _lib.check(_lib.lib().lmx_depth_templates_append(self.h, other.h))
        self._scene_shape = None

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().lmx_depth_templates_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RoughModel:
    """The mesh, the view table and the per-slot render arena of DepthTemplates.rough_pose_chain (lmx_rough_model): views[i] = (R [3, 3],
    distance in metres) belongs to template_id i of the matches -- for a bank from NativeBank.train_mesh, zip(last_side_car["R"],
    last_side_car["T"][:, 2]); D and ori_dists: the side-car's, per view.  cap_slots: the most cluster slots a call may hold;
    max_window: (w, h) of the largest render (the union of the triangles' pixel boxes) a slot can take."""

    def __init__(self, triangles, views, width, height, fx, fy, cx=None, cy=None, D=None, ori_dists=None, cap_slots=4096, max_window=None, light=MESH_LIGHT,
                 device=0):
        views = list(views)
        tri, cam, packed = _mesh_args(triangles, views, width, height, fx, fy, cx, cy, light)
        side = []
        for a in (D, ori_dists):
            a = None if a is None else np.ascontiguousarray(a, np.float64).reshape(-1)
            if a is not None and len(a) != len(views):
                raise ValueError("D and ori_dists hold one value per view")
            side.append(a)
        w, h = (width, height) if max_window is None else max_window
        self.h = C.c_void_p()
        _lib.check(_lib.lib().lmx_rough_model_create(device, tri.ctypes.data, tri.shape[0], C.byref(cam), packed.ctypes.data_as(C.POINTER(_lib.MeshView)), len(views),
                                                     side[0].ctypes.data if side[0] is not None else None, side[1].ctypes.data if side[1] is not None else None,
                                                     int(cap_slots), int(w), int(h), C.byref(self.h)))
        self.camera = (cam.fx, cam.fy, cam.cx, cam.cy)
        self.cap_slots, self.max_window, self.n_views = int(cap_slots), (int(w), int(h)), len(views)

    def device_bytes(self):
        return int(_lib.lib().lmx_rough_model_device_bytes(self.h))

    def debug_crop(self, slot):
        """Test hook (lmx_debug_rough_crop): the render the last call left in `slot`, cut to its silhouette box -> (uint16 [h, w], rect
        (x, y, w, h) in the model camera); ([0, 0], zeros) for a slot without a render."""
        buf = np.zeros(self.max_window[0] * self.max_window[1], np.uint16)
        rect = np.zeros(4, np.int32)
        _lib.check(_lib.lib().lmx_debug_rough_crop(self.h, int(slot), buf.ctypes.data, rect.ctypes.data))
        return buf[:rect[2] * rect[3]].reshape(rect[3], rect[2]).copy(), rect

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().lmx_rough_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


F2_MAX = 2048   # records per frame the device chain's LDS kernels take (csrc/lmx_internal.hpp)
F2_LARGE_MAX = 16384   # ... and its large-frame kernels; beyond it the host finishes the frame


def _finalize_buffers(n_frames, large, names):
    """The host lists of one debug_device_finalize_cluster* hook and their cut per frame.  names as _collect_buffers takes them -> (name ->
    address of a list of one row per frame, with "counts", the kernel's uint32 [n_frames][4] count words; cut(with_counts) -> list per
    frame of the tuple, each list cut to the count the kernel reported, with the frame's status behind; with_counts: (that, the words))."""
    nf = max(1, int(n_frames))
    rows = F2_LARGE_MAX if large else F2_MAX   # large: the large-frame kernel on every frame (the *_large hooks below)
    b = {k: np.zeros((nf, rows), _LIST_DTYPES[k]) for k in names if k}
    counts = np.zeros((nf, 4), np.uint32)
    ptr = {k: a.ctypes.data for k, a in b.items()}
    ptr["counts"] = counts.ctypes.data

    def cut(with_counts):
        out = []
        for f in range(n_frames):
            n_m, n_c, n_mem, status = (int(v) for v in counts[f])
            if status == 1:   # counts[0] is the record count here, not a number of matches written
                n_m = 0
            n = {"m": n_m, "d": n_m, "nd": n_m, "cl": n_c, "cc": n_c, "mem": n_mem}
            out.append(tuple(None if k is None else b[k][f, :n[k]].copy() for k in names) + (status,))
        return (out, counts) if with_counts else out
    return ptr, cut


def debug_device_finalize_cluster(records, n_frames, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min, renderer_radius_step,
                                  cluster_size_thresh=2, device=0, with_counts=False, large=False):
    """Test hook (lmx_debug_device_finalize_cluster): the kernel behind Detector.collect_clusters on a caller's RAW_MATCH_DTYPE records
    (all frames in one list, tagged by `frame`) -> list per frame of (matches, clusters, members, status), cut to the counts the
    kernel reported and otherwise as it wrote them: no host completion.  status 1 (more than F2_MAX records): all three are empty;
    status 2 (side-car / range): matches only.  with_counts: also the kernel's count words, uint32 [n_frames][4]."""
    records = np.ascontiguousarray(records, RAW_MATCH_DTYPE)
    dists, rects = _side_car(obj_origin_dists, rects)
    pp = _cluster_params(vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh)
    p, cut = _finalize_buffers(n_frames, large, ("m", "cl", "mem"))
    hook = _lib.lib().lmx_debug_device_finalize_cluster_large if large else _lib.lib().lmx_debug_device_finalize_cluster
    _lib.check(hook(device, records.ctypes.data, len(records), int(n_frames), dists.ctypes.data, rects.ctypes.data,
                    len(dists), C.byref(pp), p["m"], p["cl"], p["mem"], p["counts"]))
    return cut(with_counts)


def debug_device_finalize_cluster_depth(records, n_frames, templates, depth_frames, obj_origin_dists, rects, vote_row_col_step, renderer_radius_min,
                                        renderer_radius_step, cluster_size_thresh=2, class_index=-1, no_value=-np.inf, device=0, with_counts=False, large=False):
    """Test hook (lmx_debug_device_finalize_cluster_depth): debug_device_finalize_cluster for the kernels behind
    Detector.collect_clusters_depth; depth_frames (one per frame) become `templates`' uploaded scene.  -> list per frame of
    (matches, diffs, clusters, members, status)."""
    records = np.ascontiguousarray(records, RAW_MATCH_DTYPE)
    dists, rects = _side_car(obj_origin_dists, rects)
    pp = _cluster_params(vote_row_col_step, renderer_radius_min, renderer_radius_step, cluster_size_thresh)
    frames, imgs = _depth_images(depth_frames)
    if len(frames) != n_frames:
        raise ValueError("one depth frame per frame")
    p, cut = _finalize_buffers(n_frames, large, ("m", "d", "cl", "mem"))
    hook = _lib.lib().lmx_debug_device_finalize_cluster_large_depth if large else _lib.lib().lmx_debug_device_finalize_cluster_depth
    _lib.check(hook(device, records.ctypes.data, len(records), int(n_frames), templates.h, imgs, int(class_index),
                    float(no_value), dists.ctypes.data, rects.ctypes.data, len(dists), C.byref(pp), p["m"], p["d"], p["cl"], p["mem"], p["counts"]))
    return cut(with_counts)


def debug_device_finalize_cluster_classes(records, n_frames, classes, templates=None, class_base=None, depth_frames=None, normals=False, no_value=-np.inf,
                                          device=0, with_counts=False, large=False):
    """Test hook (lmx_debug_device_finalize_cluster_classes): the kernels behind Detector.collect_clusters_classes on a caller's records;
    classes as cluster_matches_classes takes them.  -> list per frame of (matches, diffs, ndiffs, clusters, cluster_class, members, status);
    diffs / ndiffs are None without templates / normals.  No host completion."""
    records = np.ascontiguousarray(records, RAW_MATCH_DTYPE)
    arr, keep = _class_sidecars(classes)
    score = imgs = None
    scored = templates is not None
    if scored:
        base = np.ascontiguousarray(class_base, np.int32).reshape(-1)
        frames, imgs = _depth_images(depth_frames)
        if len(frames) != n_frames or len(base) < 2:
            raise ValueError("one depth frame per frame, one class_base entry per class plus one")
        score = C.byref(_lib.ClassScore(templates.h, base.ctypes.data, len(base) - 1, int(bool(normals)), float(no_value)))
    p, cut = _finalize_buffers(n_frames, large, ("m", "d" if scored else None, "nd" if scored and normals else None, "cl", "cc", "mem"))
    hook = _lib.lib().lmx_debug_device_finalize_cluster_large_classes if large else _lib.lib().lmx_debug_device_finalize_cluster_classes
    _lib.check(hook(device, records.ctypes.data, len(records), int(n_frames), arr, len(classes), score, imgs,
                    p["m"], p.get("d"), p.get("nd"), p["cl"], p["cc"], p["mem"], p["counts"]))
    del keep
    return cut(with_counts)


def debug_device_finalize_cluster_large(*args, **kw):
    """debug_device_finalize_cluster on the large-frame kernel (lmx_debug_device_finalize_cluster_large): every frame, whatever its size, in
    rows of F2_LARGE_MAX; status 1 only beyond F2_LARGE_MAX records, status 2 also for a ring outside -2^17 .. 2^17 - 1."""
    return debug_device_finalize_cluster(*args, large=True, **kw)


def debug_device_finalize_cluster_large_depth(*args, **kw):
    """debug_device_finalize_cluster_depth on the large-frame kernel (lmx_debug_device_finalize_cluster_large_depth)."""
    return debug_device_finalize_cluster_depth(*args, large=True, **kw)


def debug_device_finalize_cluster_large_classes(*args, **kw):
    """debug_device_finalize_cluster_classes on the large-frame kernels (lmx_debug_device_finalize_cluster_large_classes); status 2 also for
    a ring outside -2^13 .. 2^13 - 1."""
    return debug_device_finalize_cluster_classes(*args, large=True, **kw)


GATHER_HEADER_BYTES = 64


def merge_gathered(blocks, n_ranks, block_stride, capacity_records, n_frames, cap_total=1 << 16, frame_groups=1):
    """Host merge (C) of gathered per-rank blocks -> list (per frame) of final matches in upstream output order.  frame_groups > 1: the ranks
    form a frame_groups x template_shards grid (rank k = group k // R, shard k % R) and a rank's records carry frame indices local to its group."""
    blocks = np.ascontiguousarray(blocks, np.uint8)
    out = np.zeros(cap_total, MATCH_DTYPE)
    offs = (C.c_size_t * (n_frames + 1))()
    _lib.check(_lib.lib().lmx_merge_gathered_groups(blocks.ctypes.data, n_ranks, block_stride, capacity_records, n_frames, frame_groups,
                                                    out.ctypes.data, cap_total, offs))
    return [out[offs[f]:offs[f + 1]].copy() for f in range(n_frames)]


def merge_raw(records, cap=1 << 16):
    """Host merge of gathered raw records of ONE frame -> final matches (std::sort + std::unique, upstream order)."""
    records = np.ascontiguousarray(records, RAW_MATCH_DTYPE)
    out = np.zeros(cap, MATCH_DTYPE)
    n = C.c_size_t()
    _lib.check(_lib.lib().lmx_merge_raw(records.ctypes.data, len(records), out.ctypes.data, cap, C.byref(n)))
    return out[:n.value].copy()


def linemod_detection(detector, sources, threshold):
    """Same shape as rgbdDetector::linemod_detection (/root/reference/src/rgbdDetector.cpp:31-34): forwards to
    match(sources, threshold, matches, class_ids={}, no quantized-image output)."""
    return detector.match(sources, threshold, ())
