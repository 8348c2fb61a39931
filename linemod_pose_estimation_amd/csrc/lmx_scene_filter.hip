// The scene's depth outlier filter on the device (lmx_depth_templates_set_scene_filter; the definition: lmx_scene_filter.hpp).  Two kernels,
// launched by lmx_verify.hip once per scene on the object's stream, a u32 score map between them:
//
//   k_scene_filter_score   workgroups of 256 lanes take 32 x 8 tiles of a frame in turn (blockIdx.x, + gridDim.x, ..; blockIdx.y: the frame).
//                  The points of the tile and of its halo of r pixels are converted once and kept in LDS as three int32 planes
//                  ((32 + 2r) x (8 + 2r) entries each: 12144 bytes at r = 7); z == 0 marks a pixel without a point, which is also what
//                  lies outside the image.  One lane scores one pixel with sf::score_pixel: every walk of the window reads LDS, no list of
//                  distances exists, so there is no per-lane array and no scratch.  The frame's sums are integers: per-lane sums over the
//                  workgroup's tiles, wave shuffles, LDS across the four waves, then five 64-bit vector atomics per workgroup -- the result
//                  does not depend on their order.
//   k_scene_filter_apply   one pixel per lane: every lane forms the threshold from the frame's finished sums (sf::threshold_of: a handful of
//                  double operations), reads its score and its depth and writes the filtered depth; the removed pixels are counted the
//                  same way, one atomic per workgroup.  Lane 0 of workgroup 0 stores the threshold.
//
// The score map costs 4 bytes written and read per pixel; scoring a pixel again in the second kernel instead would cost every walk of its
// window a second time (a few thousand LDS reads), so the map stands.  Plain C++ and vector memory operations throughout.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lmx_scene_filter.hpp"

namespace lmx {
namespace {

using sf::kTileW;
using sf::kTileH;
constexpr int kMaxLdsW = kTileW + 2 * sf::kMaxRadius, kMaxLdsH = kTileH + 2 * sf::kMaxRadius;
constexpr int kLdsPoints = kMaxLdsW * kMaxLdsH;
static_assert(3 * kLdsPoints * sizeof(int32_t) < 12 * 1024, "the tile's points stay under 12 KiB of LDS");

// The sum of v over the workgroup, valid in thread 0.  part: [4] of LDS; two barriers.
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* part) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();   // whoever still reads part from the previous sum is done
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void k_scene_filter_score(const uint16_t* __restrict__ scene, int W, int H, const sf::Params P, uint32_t* __restrict__ score,
                                                            sf::Info* __restrict__ info) {
  __shared__ int32_t px[kLdsPoints], py[kLdsPoints], pz[kLdsPoints];
  __shared__ unsigned long long part[4];
  const size_t frame = (size_t)blockIdx.y * H * W;
  const uint16_t* src = scene + frame;
  uint32_t* dst = score + frame;
  const int r = P.radius, lw = kTileW + 2 * r, lh = kTileH + 2 * r;
  const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
  const pr::Inverse inv = pr::inverse_of(P.cam);
  const int tid = threadIdx.x, tx = tid & (kTileW - 1), ty = tid / kTileW;
  unsigned long long n_valid = 0, n_sparse = 0, n_scored = 0, sum_q = 0, sum_qq = 0;
  for (int tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    __syncthreads();   // the previous tile's points are no longer read
    for (int q = tid; q < lw * lh; q += 256) {
      const int ly = q / lw, lx = q - ly * lw, X = x0 - r + lx, Y = y0 - r + ly;
      const bool inside = X >= 0 && Y >= 0 && X < W && Y < H;
      int32_t p[3];
      sf::point_of(P.cam, inv, X, Y, inside ? src[(size_t)Y * W + X] : (uint16_t)0, p);
      px[q] = p[0]; py[q] = p[1]; pz[q] = p[2];
    }
    __syncthreads();
    const int X = x0 + tx, Y = y0 + ty;
    if (X < W && Y < H) {
      const uint16_t s = src[(size_t)Y * W + X];
      uint32_t sc = sf::kInvalid;
      if (s != 0) {
        const int at = (ty + r) * lw + (tx + r);   // every neighbour's entry lies within the lw x lh entries written above
        const int32_t c[3] = {px[at], py[at], pz[at]};
        sc = sf::kSparse;
        if (c[2] != 0)
          sc = sf::score_pixel(c, s, r, P.k, [&](int32_t dx, int32_t dy, int32_t N[3]) {
            const int o = at + dy * lw + dx;
            N[0] = px[o]; N[1] = py[o]; N[2] = pz[o];
          });
        n_valid += 1;
        if (sc == sf::kSparse) {
          n_sparse += 1;
        } else {
          n_scored += 1; sum_q += sc; sum_qq += (unsigned long long)sc * sc;
        }
      }
      dst[(size_t)Y * W + X] = sc;
    }
  }
  sf::Info* out = info + blockIdx.y;
  const unsigned long long v[5] = {n_valid, n_sparse, n_scored, sum_q, sum_qq};
  int64_t* const field[5] = {&out->n_valid, &out->n_sparse, &out->n_scored, &out->sum_q, &out->sum_qq};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned long long total = block_sum(v[k], part);
    if (tid == 0 && total != 0) atomicAdd(reinterpret_cast<unsigned long long*>(field[k]), total);
  }
}

__global__ __launch_bounds__(256) void k_scene_filter_apply(const uint16_t* __restrict__ scene, const uint32_t* __restrict__ score, int W, int H, double stddev_mul,
                                                            uint16_t* __restrict__ filtered, sf::Info* __restrict__ info) {
  __shared__ unsigned long long part[4];
  const size_t frame = (size_t)blockIdx.y * H * W;
  sf::Info* out = info + blockIdx.y;
  const double thr = sf::threshold_of(out->n_scored, out->sum_q, out->sum_qq, stddev_mul);   // final: the scoring kernel ended in front of this one
  const int n = W * H;   // <= sf::kMaxFramePixels
  unsigned long long removed = 0;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
    const uint32_t sc = score[frame + q];
    const bool keep = sf::kept(sc, thr);
    removed += sc <= (uint32_t)sf::kMaxQ && !keep ? 1u : 0u;
    filtered[frame + q] = keep ? scene[frame + q] : (uint16_t)0;
  }
  const unsigned long long total = block_sum(removed, part);
  if (threadIdx.x == 0) {
    if (total != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&out->n_removed), total);
    if (blockIdx.x == 0) out->threshold = thr;
  }
}

}  // namespace

void launch_scene_filter_score(hipStream_t s, const uint16_t* scene, int32_t n_frames, int32_t W, int32_t H, const sf::Params& P, uint32_t* score, sf::Info* info) {
  const int tiles = ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH);
  hipLaunchKernelGGL(k_scene_filter_score, dim3((unsigned)std::min(tiles, sf::kScoreGridCap), (unsigned)n_frames), dim3(256), 0, s, scene, W, H, P, score, info);
}

void launch_scene_filter_apply(hipStream_t s, const uint16_t* scene, const uint32_t* score, int32_t n_frames, int32_t W, int32_t H, double stddev_mul, uint16_t* filtered,
                               sf::Info* info) {
  const unsigned gx = (unsigned)std::min<size_t>(((size_t)W * H + 255) / 256, (size_t)sf::kApplyGridCap);
  hipLaunchKernelGGL(k_scene_filter_apply, dim3(gx, (unsigned)n_frames), dim3(256), 0, s, scene, score, W, H, stddev_mul, filtered, info);
}

}  // namespace lmx
