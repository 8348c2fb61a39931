// Mesh rasteriser on the device: the renderer half of the reference's trainer (Renderer3d + RendererIterator::render as
// src/renderer.cpp:239-275 uses them), writing a batch of views straight into device memory for the batched trainer (lmx_train.cpp) and for
// lmx_mesh_render.  The arithmetic is lmx_mesh_raster.hpp (= meshraster.c, double, written order); this file is the parallel shape:
//
//   k_mesh_init    per view: clears the state words (validity, boxes)
//   k_mesh_setup   one lane per (view, triangle): projects it ONCE (u, v, 1/Z, 1/area, gray, clamped bounding box) into a work record and
//                  folds its box into the view's union box (LDS reduction, then one atomic set per workgroup)
//   k_mesh_raster  one workgroup per (view, 32x8 tile), one lane per pixel.  Tiles outside the union box only write zeros.  The others walk
//                  the view's records in chunks of 256: every lane tests one record's box against the tile, the hits are compacted IN INDEX
//                  ORDER into LDS (wave ballots + a 4-entry scan), then every lane walks the staged records against its pixel centre.  A
//                  lane sees the triangles in ascending index and replaces its z only on a strict <, so the lowest index wins among equal z
//                  without atomics, whatever the scheduling.  The silhouette boxes (level 0 and the pyramid levels' nearest-neighbour
//                  sub-samplings of the mask) are min/max reductions: LDS atomics, then one global atomic set per workgroup.
//   k_mesh_pack    per (view, level): copies the window the trainer's host half looks at (silhouette box grown by 2) of labels, magnitudes
//                  and mask into the view's slot of a pinned host buffer.
// No workgroup waits for another; every dependency is a kernel boundary on one stream.  The set-up body and the tile walk are
// lmx_mesh_device.hpp's mesh_setup and mesh_tile_walk, which lmx_rough.hip runs per cluster slot.
#include <cmath>
#include <cstring>

#include "lmx_mesh_device.hpp"

namespace lmx {
namespace {

__global__ __launch_bounds__(64) void k_mesh_init(int32_t* __restrict__ state, int n_views) {
  const int v = blockIdx.x, i = threadIdx.x;
  if (v >= n_views || i >= kMeshStateWords) return;
  state[(size_t)v * kMeshStateWords + i] = mesh_state_clear(i, 4 + 4 * kMaxLevels);   // the union box and every level's
}

__global__ __launch_bounds__(256) void k_mesh_setup(const double* __restrict__ tri, int n_tri, mr::Camera cam, const double* __restrict__ views,
                                                    mr::Tri* __restrict__ work, int32_t* __restrict__ state) {
  const int v = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  mesh_setup(tri, n_tri, cam, views + (size_t)v * 10, work + (size_t)v * n_tri, state + (size_t)v * kMeshStateWords, t);
}

__global__ __launch_bounds__(256) void k_mesh_raster(const mr::Tri* __restrict__ work, int n_tri, int W, int H, int n_levels, int32_t* __restrict__ state,
                                                     uint8_t* __restrict__ gray, uint16_t* __restrict__ depth, uint8_t* __restrict__ mask) {
  __shared__ mr::Tri s_tri[256];
  __shared__ int s_wave[4];
  __shared__ int s_lbox[kMaxLevels][4];
  const int v = blockIdx.z, tid = threadIdx.x;
  int32_t* st = state + (size_t)v * kMeshStateWords;
  if (st[MS_INVALID]) return;   // the call fails: nothing of this view is used
  const int tx0 = blockIdx.x * MR_TW, ty0 = blockIdx.y * MR_TH;
  const int x = tx0 + (tid & (MR_TW - 1)), y = ty0 + tid / MR_TW;
  const bool inside = x < W && y < H;
  const size_t o = ((size_t)v * H + (inside ? y : 0)) * W + (inside ? x : 0);
  const int ux0 = st[MS_UNION + 0], uy0 = st[MS_UNION + 1], ux1 = st[MS_UNION + 2], uy1 = st[MS_UNION + 3];
  const int tx1 = min(tx0 + MR_TW, W) - 1, ty1 = min(ty0 + MR_TH, H) - 1;
  if (ux1 < tx0 || ux0 > tx1 || uy1 < ty0 || uy0 > ty1) {   // (an empty union box has ux1 = -1 < tx0)
    if (inside) {
      if (gray) gray[o] = 0;
      if (depth) depth[o] = 0;
      if (mask) mask[o] = 0;
    }
    return;
  }
  if (tid < 4 * kMaxLevels) s_lbox[tid >> 2][tid & 3] = (tid & 2) ? -1 : MR_BIG;
  const MeshBest best = mesh_tile_walk<true>(work + (size_t)v * n_tri, n_tri, tx0, ty0, tx1, ty1, x, y, inside, s_tri, s_wave);
  const bool cov = inside && best.z < INFINITY;
  if (inside) {
    const uint16_t dmm = cov ? mr::depth_mm(best.z) : (uint16_t)0;
    if (gray) gray[o] = cov ? (uint8_t)best.gray : (uint8_t)0;
    if (depth) depth[o] = dmm;
    if (mask) mask[o] = cov ? 255 : 0;
    if (cov && x == W / 2 && y == H / 2) st[MS_CENTRE_DEPTH] = dmm;
  }
  // silhouette boxes: level l's mask is mask(y << l, x << l)
  if (cov) {
    for (int l = 0; l < n_levels; ++l) {
      if ((x | y) & ((1 << l) - 1)) break;
      const int xl = x >> l, yl = y >> l;
      if (xl >= (W >> l) || yl >= (H >> l)) break;
      atomicMin(&s_lbox[l][0], xl); atomicMin(&s_lbox[l][1], yl); atomicMax(&s_lbox[l][2], xl); atomicMax(&s_lbox[l][3], yl);
    }
  }
  __syncthreads();
  if (tid < 4 * n_levels) {
    const int l = tid >> 2, k = tid & 3, val = s_lbox[l][k];
    if (s_lbox[l][2] >= 0) {
      if (k < 2) atomicMin(&st[MS_LEVEL + 4 * l + k], val);
      else atomicMax(&st[MS_LEVEL + 4 * l + k], val);
    }
  }
}

__global__ __launch_bounds__(256) void k_mesh_pack(MeshPackArgs a) {
  const int v = blockIdx.z, l = blockIdx.y;
  const int32_t* st = a.state + (size_t)v * kMeshStateWords;
  if (st[MS_INVALID]) return;
  const int wl = a.W >> l, hl = a.H >> l;
  // the window of every level up to this one (the slot lays the levels out back to back)
  size_t off = 0;
  int wx0 = 0, wy0 = 0, ww = 0, wh = 0;
  for (int k = 0; k <= l; ++k) {
    if (k > 0) off += mesh_pack_level_bytes(ww, wh, a.n_mod, a.n_cg);
    mesh_window(st + MS_LEVEL + 4 * k, a.W >> k, a.H >> k, &wx0, &wy0, &ww, &wh);
  }
  uint8_t* out = a.out + (size_t)v * a.slot_bytes + off;
  const size_t n = (size_t)ww * wh, fpx = (size_t)wl * hl, px0 = (size_t)a.W * a.H;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int yy = (int)(i / ww), xx = (int)(i - (size_t)yy * ww);
    const int sx = wx0 + xx, sy = wy0 + yy;
    uint8_t* p = out;
    for (int m = 0; m < a.n_mod; ++m)
      if (a.mag[l][m]) { reinterpret_cast<float*>(p)[i] = a.mag[l][m][(size_t)v * fpx + (size_t)sy * wl + sx]; p += n * 4; }
    for (int m = 0; m < a.n_mod; ++m) {
      // ColorGradient: the level's own label image; DepthNormal: level 0's labels sub-sampled (upstream's nearest-neighbour chain
      // dst(y, x) = src(2y, 2x), i.e. level 0 at (y << l, x << l))
      p[i] = a.mag[l][m] ? a.quant[l][m][(size_t)v * fpx + (size_t)sy * wl + sx] : a.quant[0][m][(size_t)v * px0 + (size_t)(sy << l) * a.W + (sx << l)];
      p += n;
    }
    p[i] = a.mask0[(size_t)v * px0 + (size_t)(sy << l) * a.W + (sx << l)];
  }
}

}  // namespace

void launch_mesh_raster(hipStream_t s, const double* d_tri, int n_tri, const mr::Camera& cam, const double* d_views, int n_views, int n_levels,
                        mr::Tri* d_work, int32_t* d_state, uint8_t* gray, uint16_t* depth, uint8_t* mask) {
  hipLaunchKernelGGL(k_mesh_init, dim3((unsigned)n_views), dim3(64), 0, s, d_state, n_views);
  hipLaunchKernelGGL(k_mesh_setup, dim3((unsigned)((n_tri + 255) / 256), (unsigned)n_views), dim3(256), 0, s, d_tri, n_tri, cam, d_views, d_work, d_state);
  const dim3 grid((unsigned)((cam.W + MR_TW - 1) / MR_TW), (unsigned)((cam.H + MR_TH - 1) / MR_TH), (unsigned)n_views);
  hipLaunchKernelGGL(k_mesh_raster, grid, dim3(256), 0, s, d_work, n_tri, cam.W, cam.H, n_levels, d_state, gray, depth, mask);
}

void launch_mesh_pack(hipStream_t s, const MeshPackArgs& a, int n_views) {
  hipLaunchKernelGGL(k_mesh_pack, dim3(16, (unsigned)a.n_levels, (unsigned)n_views), dim3(256), 0, s, a);
}

// Argument checks shared by lmx_mesh_render and lmx_bank_train_mesh; fills the device form of the camera.
lmx_status mesh_check_args(const char* what, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam, const lmx_mesh_view* views,
                           int32_t n_views, mr::Camera* out) {
  if (!triangles || !cam || !views) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  if (n_triangles <= 0 || n_triangles > (1 << 22)) { set_error("%s: n_triangles = %d (expected 1 .. %d)", what, n_triangles, 1 << 22); return LMX_ERR_INVALID_ARG; }
  if (n_views < 0) { set_error("%s: n_views = %d", what, n_views); return LMX_ERR_INVALID_ARG; }
  const bool cam_finite = std::isfinite(cam->fx) && std::isfinite(cam->fy) && std::isfinite(cam->cx) && std::isfinite(cam->cy);
  if (cam->width <= 0 || cam->height <= 0 || cam->width > 16384 || cam->height > 16384 || !cam_finite || cam->fx == 0.0 || cam->fy == 0.0) {
    set_error("%s: camera %dx%d with focal lengths (%g, %g), centre (%g, %g) is not usable", what, cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy);
    return LMX_ERR_INVALID_ARG;
  }
  double l[3];
  mr::normalise_light(cam->light, l);
  if (!(std::isfinite(l[0]) && std::isfinite(l[1]) && std::isfinite(l[2]))) { set_error("%s: the camera's light direction must be finite and non-zero", what); return LMX_ERR_INVALID_ARG; }
  for (int32_t v = 0; v < n_views; ++v) {
    bool ok = std::isfinite(views[v].distance);
    for (int k = 0; k < 9; ++k) ok = ok && std::isfinite(views[v].R[k]);
    if (!ok) { set_error("%s: view %d has a non-finite rotation or distance", what, v); return LMX_ERR_INVALID_ARG; }
  }
  for (int64_t i = 0; i < (int64_t)n_triangles * 9; ++i)
    if (!std::isfinite(triangles[i])) { set_error("%s: triangle %d has a non-finite coordinate", what, (int)(i / 9)); return LMX_ERR_INVALID_ARG; }
  *out = mr::Camera{cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy, l[0], l[1], l[2]};
  return LMX_OK;
}

// meshraster.c's "return -1": a vertex at Z <= 0.01.  The same expression the device evaluates (no contraction), on the host, so that a call
// with such a view fails before anything is rendered or trained.  -> the first such view, or -1.
int mesh_first_invalid_view(const double* triangles, int32_t n_triangles, const lmx_mesh_view* views, int32_t n_views) {
  for (int32_t v = 0; v < n_views; ++v) {
    const double* R = views[v].R;
    for (int64_t i = 0; i < (int64_t)n_triangles * 3; ++i) {
      const double* q = triangles + i * 3;
      const double Z = R[6] * q[0] + R[7] * q[1] + R[8] * q[2] + views[v].distance;
      if (Z <= 0.01) return v;
    }
  }
  return -1;
}

}  // namespace lmx

#define MESH_HIP(expr)                                                                             \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      lmx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
      st = e_ == hipErrorNoDevice ? LMX_ERR_NO_DEVICE : LMX_ERR_HIP;                               \
      goto done;                                                                                   \
    }                                                                                              \
  } while (0)

extern "C" lmx_status lmx_mesh_render(int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam,
                                      const lmx_mesh_view* views, int32_t n_views, uint8_t* gray, uint16_t* depth_mm, uint8_t* mask, int32_t* rects) {
  return lmx::guarded("lmx_mesh_render", [&]() -> lmx_status {
    using namespace lmx;
    mr::Camera dc;
    lmx_status st = mesh_check_args("lmx_mesh_render", triangles, n_triangles, cam, views, n_views, &dc);
    if (st != LMX_OK || n_views == 0) return st;
    const int bad = mesh_first_invalid_view(triangles, n_triangles, views, n_views);
    if (bad >= 0) { set_error("lmx_mesh_render: view %d puts a vertex at or behind the camera (Z <= 0.01)", bad); return LMX_ERR_INVALID_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
    static_assert(sizeof(lmx_mesh_view) == 10 * sizeof(double), "lmx_mesh_view is read as 10 doubles");
    const size_t px = (size_t)dc.W * dc.H;
    const int B = std::min<int>(n_views, 32);
    double *d_tri = nullptr, *d_views = nullptr;
    mr::Tri* d_work = nullptr;
    int32_t* d_state = nullptr;
    uint8_t *d_gray = nullptr, *d_mask = nullptr;
    uint16_t* d_depth = nullptr;
    hipStream_t s = nullptr;
    std::vector<int32_t> state((size_t)B * kMeshStateWords);
    {
      MESH_HIP(hipSetDevice(device));
      MESH_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      MESH_HIP(hipMalloc(&d_tri, (size_t)n_triangles * 9 * sizeof(double)));
      MESH_HIP(hipMalloc(&d_views, (size_t)B * 10 * sizeof(double)));
      MESH_HIP(hipMalloc(&d_work, (size_t)B * n_triangles * sizeof(mr::Tri)));
      MESH_HIP(hipMalloc(&d_state, state.size() * 4));
      if (gray) MESH_HIP(hipMalloc(&d_gray, px * B));
      if (depth_mm) MESH_HIP(hipMalloc(&d_depth, px * B * 2));
      if (mask) MESH_HIP(hipMalloc(&d_mask, px * B));
      MESH_HIP(hipMemcpyAsync(d_tri, triangles, (size_t)n_triangles * 9 * sizeof(double), hipMemcpyHostToDevice, s));
      for (int first = 0; first < n_views; first += B) {
        const int n = std::min(B, n_views - first);
        MESH_HIP(hipMemcpyAsync(d_views, views + first, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice, s));
        launch_mesh_raster(s, d_tri, n_triangles, dc, d_views, n, 1, d_work, d_state, d_gray, d_depth, d_mask);
        MESH_HIP(hipGetLastError());
        MESH_HIP(hipMemcpyAsync(state.data(), d_state, (size_t)n * kMeshStateWords * 4, hipMemcpyDeviceToHost, s));
        if (gray) MESH_HIP(hipMemcpyAsync(gray + (size_t)first * px, d_gray, px * n, hipMemcpyDeviceToHost, s));
        if (depth_mm) MESH_HIP(hipMemcpyAsync(depth_mm + (size_t)first * px, d_depth, px * n * 2, hipMemcpyDeviceToHost, s));
        if (mask) MESH_HIP(hipMemcpyAsync(mask + (size_t)first * px, d_mask, px * n, hipMemcpyDeviceToHost, s));
        MESH_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i) {
          const int32_t* w = &state[(size_t)i * kMeshStateWords];
          if (w[MS_INVALID]) { set_error("lmx_mesh_render: view %d puts a vertex at or behind the camera (Z <= 0.01)", first + i); st = LMX_ERR_INVALID_ARG; goto done; }
          if (rects) {
            int32_t* r = rects + (size_t)(first + i) * 4;
            const int32_t* b = w + MS_LEVEL;
            if (b[2] >= 0) { r[0] = b[0]; r[1] = b[1]; r[2] = b[2] - b[0] + 1; r[3] = b[3] - b[1] + 1; }
            else { r[0] = r[1] = r[2] = r[3] = 0; }
          }
        }
      }
    }
  done:
    if (s) (void)hipStreamSynchronize(s);
    (void)hipFree(d_tri); (void)hipFree(d_views); (void)hipFree(d_work); (void)hipFree(d_state); (void)hipFree(d_gray); (void)hipFree(d_depth); (void)hipFree(d_mask);
    if (s) (void)hipStreamDestroy(s);
    return st;
  });
}
