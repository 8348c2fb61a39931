// Depth outlier filter of the scene ahead of the pose stages (lmx_depth_templates_set_scene_filter, include/lmx.h): the arithmetic of one
// pixel and one frame, shared by the HIP kernels (lmx_scene_filter.hip, k_scene_filter_score / k_scene_filter_apply) and -- compiled with
// LMX_SF_HOST -- by plain CPU builds (tests/cpp/scene_filter_host.cpp).  The stage stands where the reference runs
// statisticalOutlierRemoval(scene_pc, 50, 1.0) on a cluster's scene cloud (src/rgbdDetector.cpp:836, :1435-1445, PCL's filter); PCL is not
// part of the reference, so the definition below is this repository's own: PCL's filter restated on the pixel grid (DESIGN.md section 7
// lists the deviations).  Integers throughout but for the back-projection and the threshold, which use + - * / sqrt rint on doubles in the
// written order (build with -ffp-contract=off), so that the CPU build and gfx950 agree bit for bit.  This comment is the specification;
// tests/scene_filter_cases.py restates it in numpy.
//
// INPUT  a scene depth image s[H][W] (uint16 mm, 0 = no measurement) of at most 2^22 pixels, the scene camera (fx, fy, cx, cy), a window
//   radius r in 1..7, a neighbour count k in 1..(2r+1)^2 - 1 and a multiplier stddev_mul in [0, 16].
//
// POINTS  A pixel (X, Y) with s != 0 is VALID.  Q = back(scene, X, Y, s), the expression of lmx_pose_refine.hpp with the reciprocals
//   1 / fx, 1 / fy taken once.  A valid pixel with |Q.x| > 2^21 or |Q.y| > 2^21 (a comparison a NaN fails too) is FAR: it is farther than
//   any pair's partner of a pass of the refinement, it has no point and is nobody's neighbour.  Every other valid pixel has the point
//   P = llrint(16 Q) in ticks of 1/16 mm, which fits int32; P.z = 16 s > 0.
//
// NEIGHBOURS  of a valid pixel with a point: the other pixels (X + dx, Y + dy), |dx|, |dy| <= r, that lie inside the image, have a point P'
//   and satisfy |D.x|, |D.y|, |D.z| <= 2^14 for D = P' - P (the 1024 mm of pr::kMaxDistMm; |D|^2 <= 3 * 2^28 stays inside 32 bits).
//   The distance of a neighbour is d = floor(sqrt(|D|^2)), an integer.  A valid pixel that is FAR or has fewer than k neighbours is
//   SPARSE: it is removed and stays out of the statistics.
//
// SCORE  of every other valid pixel: S = the sum of its k smallest d (ties have equal values, so the sum does not depend on an order);
//   q = min((S << 16) / (k * s), 2^20 - 1), a truncating int64 division: the mean neighbour distance over the pixel's own depth, scaled by
//   2^20.  On a clean surface that ratio is about c / f at any depth, which is what gives statistics over a whole frame a meaning.
//
// STATISTICS  per frame, over the scored pixels, as int64:  n, sum q, sum q^2  (2^22 pixels of q^2 < 2^40 stay below 2^63).
//
// THRESHOLD  n < 2: thr = 2^20, which every q passes.  Otherwise, in double, in this order:
//     mean = (double)sum_q / (double)n
//     var  = ((double)sum_qq - ((double)sum_q * (double)sum_q) / (double)n) / ((double)n - 1.0);   var < 0 counts as 0
//     thr  = mean + stddev_mul * sqrt(var)
//   A scored pixel is KEPT iff (double)q <= thr, else REMOVED.
//
// OUTPUT  filtered[Y][X] = s where the pixel is kept, else 0, and the record
//     n_valid, n_sparse, n_scored, n_removed, sum_q, sum_qq (int64), threshold (double)
//   n_valid = n_sparse + n_scored; n_removed counts the scored pixels above the threshold, so n_scored - n_removed pixels are left.
//
// HOW THE SCORE IS FOUND (score_pixel; any way that gives S is as good)  No list of distances is kept: the k-th smallest distance T is
//   the smallest t whose count #{|D|^2 < (t + 1)^2} reaches k, found by bisection between 0 and the largest d of the window (at most 15
//   steps, d < 2^15); one more walk sums the d < T and adds (k - their count) * T.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifdef LMX_SF_HOST
#ifndef LMX_PR_HOST
#define LMX_PR_HOST
#endif
#define LMX_SF_FN inline
#else
#define LMX_SF_FN __host__ __device__ __forceinline__
#endif

#include "lmx_pose_refine.hpp"

#ifdef LMX_SF_HOST
#include <vector>
#endif

namespace lmx {
namespace sf {

constexpr int32_t kMaxRadius = 7;
constexpr double kMaxStddevMul = 16.0;
constexpr int32_t kMaxDiffTicks = 1 << 14;
constexpr int64_t kMaxQ = ((int64_t)1 << 20) - 1;
constexpr double kKeepAll = 1048576.0;                      // the threshold of a frame with fewer than two scored pixels
constexpr int64_t kMaxFramePixels = (int64_t)1 << 22;
constexpr uint32_t kInvalid = 0xffffffffu, kSparse = 0xfffffffeu;   // what a score map holds for a pixel without a score
// How lmx_scene_filter.hip spreads a frame (no part of the definition; the tests size their frames by them): a workgroup of 256 lanes scores
// tiles of kTileW x kTileH pixels, at most kScoreGridCap workgroups a frame, each taking the tiles blockIdx.x, + gridDim.x, ..; at most
// kApplyGridCap workgroups a frame apply the threshold, 256 pixels a trip.
constexpr int kTileW = 32, kTileH = 8;
constexpr int kScoreGridCap = 1024;
constexpr int kApplyGridCap = 1024;
static_assert(16 * pr::kMaxScenePointMm + (double)kMaxDiffTicks < 2147483648.0 && 16 * 65535 < INT32_MAX, "points and their differences fit int32");
static_assert(3ll * kMaxDiffTicks * kMaxDiffTicks < ((int64_t)1 << 30), "|D|^2 fits 32 bits, and isqrt32's argument stays below 2^30");
static_assert(kMaxQ * kMaxQ <= INT64_MAX / kMaxFramePixels, "sum q^2 over the largest frame fits int64");
static_assert((int64_t)(2 * kMaxRadius + 1) * (2 * kMaxRadius + 1) * 32768 < ((int64_t)1 << 24), "S << 16 fits int64 with room to spare");

struct Params {
  pr::Camera cam;
  double stddev_mul;
  int32_t radius, k;
};
struct Info {   // the bytes of lmx_scene_filter_info
  int64_t n_valid, n_sparse, n_scored, n_removed, sum_q, sum_qq;
  double threshold;
};

// null, or why the parameters are refused (a NaN fails its range)
LMX_SF_FN const char* check_params(const Params& P) {
  if (P.radius < 1 || P.radius > kMaxRadius) return "radius must lie in 1 .. 7";
  if (P.k < 1 || P.k > (2 * P.radius + 1) * (2 * P.radius + 1) - 1) return "k must lie in 1 .. (2 radius + 1)^2 - 1";
  if (!(P.stddev_mul >= 0.0 && P.stddev_mul <= kMaxStddevMul)) return "stddev_mul must lie in [0, 16]";
  const double c[4] = {P.cam.fx, P.cam.fy, P.cam.cx, P.cam.cy};
  for (int i = 0; i < 4; ++i)
    if (!(c[i] > 0.0 && c[i] <= 1.7976931348623157e308)) return "the camera's fx, fy, cx, cy must be finite and above 0";
  return nullptr;
}

// The point of pixel (X, Y); P[2] == 0: it has none (no measurement, or FAR).
LMX_SF_FN void point_of(const pr::Camera& cam, const pr::Inverse& inv, int32_t X, int32_t Y, uint16_t s, int32_t P[3]) {
  P[0] = P[1] = P[2] = 0;
  if (s == 0) return;
  double Q[3];
  pr::back(cam, inv, X, Y, s, Q);
  if (!(fabs(Q[0]) <= pr::kMaxScenePointMm) || !(fabs(Q[1]) <= pr::kMaxScenePointMm)) return;
  P[0] = (int32_t)rint(16.0 * Q[0]); P[1] = (int32_t)rint(16.0 * Q[1]); P[2] = 16 * (int32_t)s;
}

// floor(sqrt(x)) for x < 2^30: a float estimate, put right in integers
LMX_SF_FN uint32_t isqrt32(uint32_t x) {
  uint32_t r = (uint32_t)sqrtf((float)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// f(|D|^2) for every neighbour of the pixel whose point is P; win(dx, dy, N) gives the point of the pixel at that offset (N[2] == 0 for none,
// which is also what a pixel outside the image has)
template <typename Window, typename F>
LMX_SF_FN void for_neighbours(const int32_t P[3], int32_t r, const Window& win, const F& f) {
  for (int32_t dy = -r; dy <= r; ++dy)
    for (int32_t dx = -r; dx <= r; ++dx) {
      if (dx == 0 && dy == 0) continue;
      int32_t N[3];
      win(dx, dy, N);
      if (N[2] == 0) continue;
      const int32_t ax = abs(N[0] - P[0]), ay = abs(N[1] - P[1]), az = abs(N[2] - P[2]);
      if (ax > kMaxDiffTicks || ay > kMaxDiffTicks || az > kMaxDiffTicks) continue;
      f((uint32_t)(ax * ax) + (uint32_t)(ay * ay) + (uint32_t)(az * az));
    }
}

// The score of a valid pixel with the point P and the depth s: q, or kSparse.
template <typename Window>
LMX_SF_FN uint32_t score_pixel(const int32_t P[3], uint16_t s, int32_t r, int32_t k, const Window& win) {
  uint32_t n = 0, max_sq = 0;
  for_neighbours(P, r, win, [&](uint32_t sq) { n += 1; max_sq = sq > max_sq ? sq : max_sq; });
  if (n < (uint32_t)k) return kSparse;
  uint32_t lo = 0, hi = isqrt32(max_sq);
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1, lim = (mid + 1) * (mid + 1);
    uint32_t c = 0;
    for_neighbours(P, r, win, [&](uint32_t sq) { c += sq < lim ? 1u : 0u; });
    if (c >= (uint32_t)k) hi = mid; else lo = mid + 1;
  }
  const uint32_t T = lo, tt = T * T;
  uint32_t below = 0, sum = 0;
  for_neighbours(P, r, win, [&](uint32_t sq) { if (sq < tt) { below += 1; sum += isqrt32(sq); } });
  const int64_t S = (int64_t)sum + (int64_t)((uint32_t)k - below) * (int64_t)T;
  const int64_t q = (S << 16) / ((int64_t)k * (int64_t)s);
  return (uint32_t)(q > kMaxQ ? kMaxQ : q);
}

LMX_SF_FN double threshold_of(int64_t n, int64_t sum_q, int64_t sum_qq, double stddev_mul) {
  if (n < 2) return kKeepAll;
  const double N = (double)n, sq = (double)sum_q;
  const double mean = sq / N;
  double var = ((double)sum_qq - (sq * sq) / N) / (N - 1.0);
  if (!(var > 0.0)) var = 0.0;
  return mean + stddev_mul * sqrt(var);
}

LMX_SF_FN bool kept(uint32_t score, double thr) { return score <= (uint32_t)kMaxQ && (double)score <= thr; }

#ifdef LMX_SF_HOST
// One frame on the CPU: scene [H] rows of `pitch` elements, out [H][W].  The parameters passed check_params and W * H <= kMaxFramePixels.
inline void filter_frame(const uint16_t* scene, int32_t W, int32_t H, size_t pitch, const Params& P, uint16_t* out, Info* info) {
  const size_t px = (size_t)W * (size_t)H;
  std::vector<int32_t> pts(3 * px);
  std::vector<uint32_t> score(px);
  const pr::Inverse inv = pr::inverse_of(P.cam);
  for (int32_t Y = 0; Y < H; ++Y)
    for (int32_t X = 0; X < W; ++X) point_of(P.cam, inv, X, Y, scene[(size_t)Y * pitch + X], &pts[3 * ((size_t)Y * W + X)]);
  Info r = {0, 0, 0, 0, 0, 0, 0.0};
  for (int32_t Y = 0; Y < H; ++Y)
    for (int32_t X = 0; X < W; ++X) {
      const size_t at = (size_t)Y * W + X;
      const uint16_t s = scene[(size_t)Y * pitch + X];
      score[at] = kInvalid;
      if (s == 0) continue;
      r.n_valid += 1;
      const int32_t* C = &pts[3 * at];
      uint32_t sc = kSparse;
      if (C[2] != 0)
        sc = score_pixel(C, s, P.radius, P.k, [&](int32_t dx, int32_t dy, int32_t N[3]) {
          const int32_t x = X + dx, y = Y + dy;
          N[2] = 0;
          if (x < 0 || y < 0 || x >= W || y >= H) return;
          const int32_t* p = &pts[3 * ((size_t)y * W + x)];
          N[0] = p[0]; N[1] = p[1]; N[2] = p[2];
        });
      score[at] = sc;
      if (sc == kSparse) { r.n_sparse += 1; continue; }
      r.n_scored += 1; r.sum_q += sc; r.sum_qq += (int64_t)sc * sc;
    }
  r.threshold = threshold_of(r.n_scored, r.sum_q, r.sum_qq, P.stddev_mul);
  for (int32_t Y = 0; Y < H; ++Y)
    for (int32_t X = 0; X < W; ++X) {
      const size_t at = (size_t)Y * W + X;
      const bool keep = kept(score[at], r.threshold);
      if (score[at] <= (uint32_t)kMaxQ && !keep) r.n_removed += 1;
      out[at] = keep ? scene[(size_t)Y * pitch + X] : (uint16_t)0;
    }
  *info = r;
}
#endif

}  // namespace sf

#ifndef LMX_SF_HOST
// lmx_scene_filter.hip, for the n_frames W x H frames at `scene`.  score: `info` [n_frames] was zeroed on `s` in front of it; behind it
// the score map and the five sums are final.  apply, behind it on the same stream: filtered, n_removed and threshold.
void launch_scene_filter_score(hipStream_t s, const uint16_t* scene, int32_t n_frames, int32_t W, int32_t H, const sf::Params& P, uint32_t* score, sf::Info* info);
void launch_scene_filter_apply(hipStream_t s, const uint16_t* scene, const uint32_t* score, int32_t n_frames, int32_t W, int32_t H, double stddev_mul, uint16_t* filtered,
                               sf::Info* info);
#endif
}  // namespace lmx
