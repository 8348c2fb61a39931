"""Reference for per-class match thresholds, built from the oracle alone: what cv::linemod::Detector::match would produce if it passed
thresholds[class] instead of `threshold` to each matchClass call.

  1. for the classes in visiting order (the class_ids list when given, else the oracle's class order), with insertion slot s, the oracle
     matches that class alone at its own threshold (OracleDetector.match(sources, thresholds[c], class_ids=[c])) and hands out its raw
     list in insertion order (last_raw());
  2. bits 48 and up of every record's order_key become s (a one-class call always numbers its class 0);
  3. the lists are concatenated: upstream's `matches` vector after the visit;
  4. the real std::sort orders it (lmo_std_sort_perm on (similarity, template_id));
  5. std::unique drops every record equal to its predecessor in (x, y, similarity, class_index).

The candidate count of the composed call is the sum of the one-class calls' last_candidates()."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from oracle import oracle as o

FIELDS = ("x", "y", "similarity", "template_id", "class_index")
KEY_MASK = np.uint64((1 << 48) - 1)

# the inputs the composition was checked on (test_class_thresholds_host.py) and the GPU tests' smaller bank: three classes, thresholds far apart
W, H = 320, 240
CLASSES = ["a", "b", "c"]
THRESHOLDS = {"a": 90.0, "b": 78.0, "c": 84.0}
SCENE_KW = dict(n_instances=8, n_distractors=2)


def make_bank(n_per_class):
    from linemod_pose_estimation_amd import synth
    return synth.make_bank(n_per_class, seed=79, size_range=(40.0, 110.0), classes=CLASSES)


def make_frames(bank, seeds):
    """One scene per entry of `seeds`; None stands for an all-zero frame."""
    from linemod_pose_estimation_amd import synth
    frames = []
    for seed in seeds:
        fr = synth.make_scene(bank, W, H, seed=902 if seed is None else seed, **SCENE_KW)[0]
        if seed is None:
            fr = [np.zeros_like(np.ascontiguousarray(s)) for s in fr]
        frames.append(fr)
    return frames


def as_list(m):
    return list(zip(*(m[k].tolist() for k in FIELDS)))


def with_slot(raw, slot):
    r = raw.copy()
    r["order_key"] = (r["order_key"] & KEY_MASK) | (np.uint64(slot) << np.uint64(48))
    return r


def std_sort_unique(raw):
    """Steps 4 and 5 on raw records in insertion order -> the surviving records (raw layout), in output order."""
    n = len(raw)
    if n == 0:
        return raw.copy()
    sim = np.ascontiguousarray(raw["similarity"], np.float32)
    tid = np.ascontiguousarray(raw["template_id"], np.int32)
    perm = np.zeros(n, np.int32)
    o.lib().lmo_std_sort_perm(sim.ctypes.data_as(C.c_void_p), tid.ctypes.data_as(C.c_void_p), C.c_long(n), perm.ctypes.data_as(C.c_void_p))
    s = raw[perm]
    keep = np.ones(n, bool)
    same = np.ones(n - 1, bool)
    for k in ("x", "y", "similarity", "class_index"):
        same &= s[k][1:] == s[k][:-1]
    keep[1:] = ~same
    return s[keep]


def reference(od, sources, thresholds, class_ids=None, masks=None):
    """-> namespace(raw: the concatenated raw records with the visit's slots in their order_key, final: the records that survive sort + unique
    in output order, candidates: coarse candidates of the whole visit, per_class: {class id: records of `final`})."""
    names = od.class_ids()
    visit = list(class_ids) if class_ids else names
    parts, cands = [], 0
    for slot, c in enumerate(visit):
        od.match(sources, float(thresholds[c]), class_ids=[c], masks=masks)
        parts.append(with_slot(od.last_raw(), slot))
        cands += od.last_candidates()
    raw = np.concatenate(parts) if parts else np.zeros(0, o.RAW_DTYPE)
    final = std_sort_unique(raw)
    per_class = {c: final[final["class_index"] == names.index(c)] for c in visit}
    return SimpleNamespace(raw=raw, final=final, candidates=cands, per_class=per_class)


def uniform(od, sources, t):
    """The oracle's own list at one threshold for every class, and its raw records."""
    m = od.match(sources, float(t))
    return m, od.last_raw()
