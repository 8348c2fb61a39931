#!/usr/bin/env python3
"""Generates tests/golden/depth_normal_sensitive.npz: the tap tuples at which the depth quantiser's float stage can tell a correctly
rounded sqrt / divide from one that is a float32 ulp off (family S of tests/depth_cases.py), and the exact lattice points met on the
way.  The search is tests/depth_cases.py's (slices of structured and random tuples, a float64 filter, then the numpy restatement's
own sensitivity test); nothing but this repository's restatement is involved.  Arrays, one row per tuple:
  taps u16 [n, 9]   the pixel's depth and its eight neighbours in np_restatement.TAP_OFFSETS order
  dist, thr i32     distance_threshold and difference_threshold the row was found under
  sensitive, lattice bool;  slice i32: index into depth_cases.slices() of the slice that produced the row
Run from the repo root (a few minutes):  python tests/golden/make_depth_normal_sensitive.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import depth_cases as dc  # noqa: E402


def main():
    cols = dict(taps=[], dist=[], thr=[], sensitive=[], lattice=[], slice=[])
    n_cand = 0
    for k, desc in enumerate(dc.slices()):
        t, dist, thr, s, l, n = dc.search_slice(desc)
        n_cand += len(dc.candidates(desc)[0]) if "--count" in sys.argv else 0
        cols["taps"].append(t)
        cols["dist"].append(np.full(len(t), dist, np.int32))
        cols["thr"].append(np.full(len(t), thr, np.int32))
        cols["sensitive"].append(s)
        cols["lattice"].append(l)
        cols["slice"].append(np.full(len(t), k, np.int32))
        print(k, desc, len(t), int(s.sum()), int(l.sum()), flush=True)
    out = {k: np.concatenate(v) for k, v in cols.items()}
    np.savez_compressed(dc.FIXTURE, **out)
    for thr in np.unique(out["thr"]):
        m = out["thr"] == thr
        print("thr", thr, "rows", int(m.sum()), "sensitive", int(out["sensitive"][m].sum()), "lattice", int(out["lattice"][m].sum()))
    print("rows", len(out["thr"]), "sensitive", int(out["sensitive"].sum()), "candidates", n_cand, "bytes", os.path.getsize(dc.FIXTURE))


if __name__ == "__main__":
    main()
