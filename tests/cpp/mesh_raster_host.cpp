// CPU build of the mesh rasteriser's device header (linemod_pose_estimation_amd/csrc/lmx_mesh_raster.hpp under LMX_MR_HOST) for
// tests/test_mesh_raster_host.py: the same per-triangle set-up and per-pixel test the HIP kernels run, driven by a plain loop that walks the
// triangles in ascending index with a strict < (what a lane of k_mesh_raster does for its pixel).
#define LMX_MR_HOST 1
#include "lmx_mesh_raster.hpp"

#include <limits>
#include <vector>

using namespace lmx::mr;

// views: n_views x {R[9], distance}.  Outputs as lmx_mesh_render: gray u8, depth u16, mask u8 [n_views][H][W], rects int32 [n_views][4].
// Returns -1, or the index of the first invalid view (a vertex at Z <= 0.01): nothing is written for that view or any later one.
extern "C" int mr_host_render(const double* tri, int n_tri, int W, int H, double fx, double fy, double cx, double cy, const double* light,
                              const double* views, int n_views, uint8_t* gray, uint16_t* depth, uint8_t* mask, int32_t* rects) {
  Camera cam{W, H, fx, fy, cx, cy, 0, 0, 0};
  double l[3];
  normalise_light(light, l);
  cam.l0 = l[0]; cam.l1 = l[1]; cam.l2 = l[2];
  const size_t px = (size_t)W * H;
  std::vector<Tri> tris;
  std::vector<double> zbuf(px);
  std::vector<int32_t> shade(px);
  for (int vi = 0; vi < n_views; ++vi) {
    const double* R = views + (size_t)vi * 10;
    tris.clear();
    for (int t = 0; t < n_tri; ++t) {
      Tri tr;
      const int rc = setup_triangle(tri + (size_t)t * 9, R, R[9], cam, tr);
      if (rc == TRI_INVALID_VIEW) return vi;
      if (rc == TRI_OK) tris.push_back(tr);
    }
    for (size_t i = 0; i < px; ++i) { zbuf[i] = std::numeric_limits<double>::infinity(); shade[i] = 0; }
    for (const Tri& tr : tris)
      for (int y = tr.y0; y <= tr.y1; ++y)
        for (int x = tr.x0; x <= tr.x1; ++x) {
          double iz;
          if (!in_box(tr, x, y) || !cover(tr, x, y, &iz)) continue;
          const double z = 1.0 / iz;
          const size_t i = (size_t)y * W + x;
          if (z < zbuf[i]) { zbuf[i] = z; shade[i] = tr.gray; }
        }
    int xmin = W, ymin = H, xmax = -1, ymax = -1;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x, o = (size_t)vi * px + i;
        const bool cov = zbuf[i] < std::numeric_limits<double>::infinity();
        gray[o] = cov ? (uint8_t)shade[i] : 0;
        depth[o] = cov ? depth_mm(zbuf[i]) : 0;
        mask[o] = cov ? 255 : 0;
        if (cov) { if (x < xmin) xmin = x; if (x > xmax) xmax = x; if (y < ymin) ymin = y; if (y > ymax) ymax = y; }
      }
    int32_t* r = rects + (size_t)vi * 4;
    if (xmax >= 0) { r[0] = xmin; r[1] = ymin; r[2] = xmax - xmin + 1; r[3] = ymax - ymin + 1; }
    else { r[0] = r[1] = r[2] = r[3] = 0; }
  }
  return -1;
}
