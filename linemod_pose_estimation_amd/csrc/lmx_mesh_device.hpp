// The device bodies the two rasterisers share: lmx_mesh.hip (a batch of views into whole frames) and lmx_rough.hip (a slot's mean view into
// its window).  The arithmetic is lmx_mesh_raster.hpp; the kernels keep their index mapping, their early exits and their addressing.
#pragma once

#include <cmath>

#include "lmx_internal.hpp"
#include "lmx_mesh_raster.hpp"

namespace lmx {

constexpr int MR_TW = 32, MR_TH = 8;   // tile of the raster kernels: 256 lanes, a wave = two rows of 32 pixels
constexpr int MR_BIG = 0x7fffffff;

// What word i of a state row is cleared to: the n_box_words words from MS_UNION on are boxes {min, min, max, max}, the others zero.
__device__ __forceinline__ int32_t mesh_state_clear(int i, int n_box_words) {
  return (i >= MS_UNION && i < MS_UNION + n_box_words) ? (((i - MS_UNION) & 2) ? -1 : MR_BIG) : 0;
}

// One lane per triangle t of a 256-lane workgroup (every lane of the workgroup calls): projects it ONCE under view10 = {R, distance} into
// work_row[t] and folds its box into the view's union box (LDS reduction, then one atomic set per workgroup).
__device__ __forceinline__ void mesh_setup(const double* __restrict__ tri, int n_tri, const mr::Camera& cam, const double* __restrict__ view10,
                                           mr::Tri* __restrict__ work_row, int32_t* __restrict__ state_row, int t) {
  __shared__ int s_box[4], s_bad;
  if (threadIdx.x == 0) { s_box[0] = s_box[1] = MR_BIG; s_box[2] = s_box[3] = -1; s_bad = 0; }
  __syncthreads();
  if (t < n_tri) {
    double R[9];
    for (int k = 0; k < 9; ++k) R[k] = view10[k];
    mr::Tri rec;
    const int rc = mr::setup_triangle(tri + (size_t)t * 9, R, view10[9], cam, rec);
    if (rc != mr::TRI_OK) { rec = mr::Tri(); rec.x0 = 0; rec.x1 = -1; rec.y0 = 0; rec.y1 = -1; }   // an empty box: no pixel ever tests it
    if (rc == mr::TRI_INVALID_VIEW) atomicOr(&s_bad, 1);
    work_row[t] = rec;
    if (rc == mr::TRI_OK && rec.x0 <= rec.x1 && rec.y0 <= rec.y1) {
      atomicMin(&s_box[0], rec.x0); atomicMin(&s_box[1], rec.y0); atomicMax(&s_box[2], rec.x1); atomicMax(&s_box[3], rec.y1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_bad) atomicOr(&state_row[MS_INVALID], 1);
    if (s_box[2] >= 0) {
      atomicMin(&state_row[MS_UNION + 0], s_box[0]); atomicMin(&state_row[MS_UNION + 1], s_box[1]);
      atomicMax(&state_row[MS_UNION + 2], s_box[2]); atomicMax(&state_row[MS_UNION + 3], s_box[3]);
    }
  }
}

struct MeshBest { double z; int gray; };   // z: INFINITY where nothing covers the pixel; gray: with GRAY only

// The walk of one tile [tx0, tx1] x [ty0, ty1] by a 256-lane workgroup, lane tid at pixel (x, y), `inside` where that pixel exists.  The
// view's n_tri records in chunks of 256: every lane tests one record's box against the tile, the hits are compacted IN INDEX ORDER into
// s_tri (wave ballots + a 4-entry scan over s_wave), then every lane walks the staged records against its pixel centre.  A lane sees the
// triangles in ascending index and replaces its z only on a strict <, so the lowest index wins among equal z without atomics.
template <bool GRAY>
__device__ __forceinline__ MeshBest mesh_tile_walk(const mr::Tri* __restrict__ vw, int n_tri, int tx0, int ty0, int tx1, int ty1, int x, int y, bool inside,
                                                   mr::Tri* s_tri, int* s_wave) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double best_z = INFINITY, best_iz = -INFINITY;
  int best_gray = 0;
  for (int base = 0; base < n_tri; base += 256) {
    const int t = base + tid;
    bool hit = false;
    if (t < n_tri) {
      const int4 b = *reinterpret_cast<const int4*>(&vw[t].x0);   // x0, x1, y0, y1
      hit = b.x <= tx1 && b.y >= tx0 && b.z <= ty1 && b.w >= ty0 && b.x <= b.y && b.z <= b.w;
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();   // also: the previous chunk's records have been read by every lane
    int slot = __popcll(bal & ((1ull << lane) - 1ull));
    int n_hit = 0;
    for (int w = 0; w < 4; ++w) { const int c = s_wave[w]; if (w < wave) slot += c; n_hit += c; }
    if (hit) s_tri[slot] = vw[t];
    __syncthreads();
    if (inside) {
      for (int k = 0; k < n_hit; ++k) {
        const mr::Tri& tr = s_tri[k];
        double iz;
        if (!mr::in_box(tr, x, y) || !mr::cover(tr, x, y, &iz)) continue;
        // z = 1 / iz does not increase with iz: a triangle whose iz is not above the winner's cannot have a smaller z (the division is skipped)
        if (!(iz > best_iz)) continue;
        const double z = 1.0 / iz;
        if (z < best_z) { best_z = z; best_iz = iz; if (GRAY) best_gray = tr.gray; }
      }
    }
  }
  return MeshBest{best_z, best_gray};
}

}  // namespace lmx
