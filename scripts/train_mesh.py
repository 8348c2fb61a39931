#!/usr/bin/env python3
"""Train a template bank from a mesh: the counterpart of the reference's launch/start_object_renderer.launch (src/renderer.cpp).

    python scripts/train_mesh.py MESH OUT_templates.yml OUT_renderer_params.yml [options]

MESH is a triangle .npz (key `triangles`, float [n, 3, 3], metres, as in tests/golden/meshes/) or an .stl (binary or ASCII; units are taken
as metres, --scale converts).  Every view of the grid is rendered on the device and handed to addTemplate there (lmx_bank_train_mesh);
the two files are what readLinemod / readLinemodTemplateParams read.  Views: meshsynth.view_grid over the radii --radius-min ..
--radius-max in steps of --radius-step (the reference's 442-rotation pose list per radius), cut to --max-views."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linemod_pose_estimation_amd import NativeBank, meshsynth as ms  # noqa: E402


def read_stl(path):
    """-> float64 [n, 3, 3].  Binary STL: 80-byte header, uint32 count, then per triangle 12 float32 (normal, 3 vertices) + uint16;
    ASCII STL: `vertex x y z` lines, three per facet."""
    raw = open(path, "rb").read()
    if len(raw) >= 84:
        n = int(np.frombuffer(raw, "<u4", 1, 80)[0])
        if len(raw) == 84 + 50 * n:     # the size decides: binary files may start with "solid" too
            rec = np.frombuffer(raw, np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), n, 84)
            return rec["v"].astype(np.float64)
    verts = [ln.split()[1:4] for ln in raw.decode("ascii", "replace").splitlines() if ln.strip().startswith("vertex")]
    if not verts or len(verts) % 3:
        raise ValueError("%s: neither a binary STL (size != 84 + 50 n) nor an ASCII STL with 3 vertices per facet" % path)
    return np.asarray(verts, np.float64).reshape(-1, 3, 3)


def load_mesh(path):
    if path.lower().endswith(".npz"):
        return np.load(path)["triangles"].astype(np.float64)
    return read_stl(path)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("out_templates")
    ap.add_argument("out_renderer_params")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--fx", type=float, default=ms.ENSENSO["fx"])
    ap.add_argument("--fy", type=float, default=None, help="default: --fx")
    ap.add_argument("--radius-min", type=float, default=ms.ENSENSO["radius_min"])
    ap.add_argument("--radius-max", type=float, default=ms.ENSENSO["radius_max"])
    ap.add_argument("--radius-step", type=float, default=ms.ENSENSO["radius_step"])
    ap.add_argument("--max-views", type=int, default=0, help="train only the first N views of the grid")
    ap.add_argument("--modalities", default="ColorGradient,DepthNormal")
    ap.add_argument("--class-id", default="obj")
    ap.add_argument("--scale", type=float, default=1.0, help="factor from the mesh's unit to metres (0.001 for millimetres)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--device-candidates", action="store_true",
                    help="find and compact the feature candidates on the device (lmx_bank_train_mesh_opts); the bank and the side-car are the same")
    a = ap.parse_args(argv)
    tri = load_mesh(a.mesh) * a.scale
    n_r = int(round((a.radius_max - a.radius_min) / a.radius_step)) + 1
    radii = [a.radius_min + i * a.radius_step for i in range(n_r)]
    views = ms.view_grid(radii)
    if a.max_views > 0:
        views = views[:a.max_views]
    fy = a.fx if a.fy is None else a.fy
    bank = ms.empty_bank(tuple(m.strip() for m in a.modalities.split(",") if m.strip()))
    nb = NativeBank.create(bank.T, bank.modalities)
    # the iterator scalars a view LIST can state: the radii (what the cluster chain reads); n_points / angle_step / near / far stay 0
    scalars = {"renderer_radius_min": a.radius_min, "renderer_radius_max": a.radius_max, "renderer_radius_step": a.radius_step}
    meta = nb.train_mesh(tri, views, a.width, a.height, a.fx, fy, class_id=a.class_id, device=a.device, save_side_car=a.out_renderer_params,
                         side_car_scalars=scalars, device_candidates=a.device_candidates)
    nb.save_yaml(a.out_templates)
    print("train_mesh: %d triangles, %d views, %d templates -> %s, %s" % (len(tri), len(views), len(meta), a.out_templates, a.out_renderer_params))
    if a.device_candidates:
        st = nb.last_train_stats
        print("train_mesh: candidates on the device for %d views (%d through the host path), %d candidates, %.1f MB of lists" %
              (st["n_device_views"], st["n_fallback_views"], st["n_candidates"], st["list_bytes"] / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main())
