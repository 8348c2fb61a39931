// Normal-difference term of a match (lmx_normal_diff_matches, include/lmx.h): the arithmetic of one pixel's normal, one pixel pair's angle,
// one match's sums and one match's value, shared by the HIP kernels (lmx_verify.hip: k_normal_map_*, and add_vector as the inner step of
// the NORMALS forms of k_walk and k_walk_records_dev; lmx_f2.hip for value()) and -- compiled with LMX_NV_HOST -- by plain CPU builds
// (tests/cpp/normal_verify_host.cpp).
// The reference's form is depth_normal_diff_calc (src/rgbdDetector.cpp:147-359), the normal half: the mean angle between the surface normals
// of the template's rendered depth and of the scene depth over the pixels both cover.  The reference takes its normals from OpenCV's rgbd
// module (RGBD_NORMALS_METHOD_LINEMOD), which is not part of it; the definition below is this project's own (deviations).
//
// NORMAL of pixel (x, y) of a uint16-mm depth image D (reads outside the image or crop give 0).  d = D[y][x]; the pixel is INVALID iff d == 0
// or d >= distance_threshold.  Otherwise the eight taps at offsets +-5 enter DepthNormal's least squares (accum_bilateral: a tap counts iff
// |tap - d| < difference_threshold), det / ddx / ddy in 64-bit integers exactly as the depth quantiser computes them, then
//   nx = fx * (float)ddx,  ny = fy * (float)ddy,  nz = -(float)(det * d),  s = sqrtf(nx*nx + ny*ny + nz*nz)     (no contraction: -ffp-contract=off)
// invalid unless s > 0;  inv = 1.0f / s;  q_c = (int16)rintf((n_c * inv) * 16384.0f).  Stored as four int16 {qx, qy, qz, valid}: 8 bytes, all
// zeros when invalid.
//
// ANGLE of two stored normals: integer differences dx, dy, dz; c2 = dx^2 + dy^2 + dz^2 in 64 bits; c = sqrtf((float)c2);
// i = min(16384, (int)rintf(c * 0.5f)); angle_urad = table[i] with table[i] = llrint(2e6 * asin(min(1.0, i / 16384.0))): the chord -> angle map,
// built once on the host in double (build_angle_table) so that host and device read the same numbers and no transcendental function runs on
// the device.  Identical normals give exactly 0.
//
// SUMS of a match: a crop pixel counts for the normal term iff it counts for the depth term (lmx_depth_verify.hpp) and both normals are valid;
// n_normal = #counting, sum_angle_urad = the sum of their angles in 64 bits (64 x 64 pixels near pi already pass 2^32).
#pragma once

#ifdef LMX_NV_HOST
#ifndef LMX_DV_HOST
#define LMX_DV_HOST
#endif
#define LMX_NV_FN inline
#define LMX_NV_UNROLL
#include <math.h>
#else
#define LMX_NV_FN __host__ __device__ __forceinline__
#define LMX_NV_UNROLL _Pragma("unroll")
#endif

#include "lmx_depth_verify.hpp"

namespace lmx {
namespace nv {

constexpr int kTap = 5;                 // the taps of DepthNormal's least squares lie at offsets +-5
constexpr int kUnit = 16384;            // a unit normal's component scale
constexpr int kAngleTableSize = 16385;  // half chords 0 .. 16384
// How lmx_verify.hip spreads the normal maps (no part of the definition; the tests size their images by them): workgroups of 256 lanes,
// a pixel per lane and trip -- at most kFrameMapGridCap of them per scene frame, kCropMapGrid per crop (h * pitch elements).
constexpr int kFrameMapGridCap = 4096;
constexpr int kCropMapGrid = 32;

struct Params {
  float fx, fy;
  int32_t difference_threshold, distance_threshold;
};

// A stored normal as one 8-byte element: qx | qy << 16 | qz << 32 | valid << 48 (the int16 fields as unsigned halves).  0 = invalid.
typedef uint64_t Packed;
LMX_NV_FN Packed pack(int32_t qx, int32_t qy, int32_t qz) {
  return (uint64_t)(uint16_t)qx | ((uint64_t)(uint16_t)qy << 16) | ((uint64_t)(uint16_t)qz << 32) | ((uint64_t)1 << 48);
}
LMX_NV_FN bool valid(Packed n) { return (n >> 48) != 0; }
LMX_NV_FN int32_t comp(Packed n, int c) { return (int32_t)(int16_t)(uint16_t)(n >> (16 * c)); }

struct Sums {
  uint64_t sum_angle_urad;   // <= 2^28 pixels x 3141593 < 2^50
  int32_t n_normal;
};

// The normal of a pixel of depth d (valid by the caller's test: 0 < d < distance_threshold) from its eight taps, in the order
// (-5,-5) (0,-5) (5,-5) (-5,0) (5,0) (-5,5) (0,5) (5,5) of the depth quantiser.
LMX_NV_FN Packed normal_from_taps(int32_t d, const int32_t tap[8], const Params& p) {
  const int ox[8] = {-kTap, 0, kTap, -kTap, kTap, -kTap, 0, kTap};
  const int oy[8] = {-kTap, -kTap, -kTap, 0, 0, kTap, kTap, kTap};
  int64_t A0 = 0, A1 = 0, A3 = 0, b0 = 0, b1 = 0;
  for (int k = 0; k < 8; ++k) {
    const int64_t delta = (int64_t)tap[k] - (int64_t)d;
    const int64_t f = (delta < 0 ? -delta : delta) < (int64_t)p.difference_threshold ? 1 : 0;
    const int64_t fi = f * ox[k], fj = f * oy[k];
    A0 += fi * ox[k]; A1 += fi * oy[k]; A3 += fj * oy[k];
    b0 += fi * delta; b1 += fj * delta;
  }
  const int64_t det = A0 * A3 - A1 * A1;
  const int64_t ddx = A3 * b0 - A1 * b1;
  const int64_t ddy = -A1 * b0 + A0 * b1;
  const float nx = p.fx * (float)ddx;
  const float ny = p.fy * (float)ddy;
  const float nz = -(float)(det * (int64_t)d);
  const float s = sqrtf(nx * nx + ny * ny + nz * nz);
  if (!(s > 0.0f)) return 0;
  const float inv = 1.0f / s;
  const int32_t qx = (int32_t)rintf((nx * inv) * (float)kUnit);
  const int32_t qy = (int32_t)rintf((ny * inv) * (float)kUnit);
  const int32_t qz = (int32_t)rintf((nz * inv) * (float)kUnit);
  return pack(qx, qy, qz);
}

// Pixel (x, y) of the w x h image img (rows of `pitch` elements); reads outside [0, w) x [0, h) give 0 and touch no memory.
LMX_NV_FN int32_t depth_or_zero(const uint16_t* img, int32_t w, int32_t h, size_t pitch, int32_t x, int32_t y) {
  return (x >= 0 && x < w && y >= 0 && y < h) ? (int32_t)img[(size_t)y * pitch + (size_t)x] : 0;
}

// The normal of pixel (x, y), 0 <= x < w, 0 <= y < h.
LMX_NV_FN Packed normal_at(const uint16_t* img, int32_t w, int32_t h, size_t pitch, int32_t x, int32_t y, const Params& p) {
  const int32_t d = (int32_t)img[(size_t)y * pitch + (size_t)x];
  if (d == 0 || d >= p.distance_threshold) return 0;
  int32_t tap[8];
  int k = 0;
  for (int j = -1; j <= 1; ++j)
    for (int i = -1; i <= 1; ++i)
      if (i != 0 || j != 0) tap[k++] = depth_or_zero(img, w, h, pitch, x + i * kTap, y + j * kTap);
  return normal_from_taps(d, tap, p);
}

// Index into the angle table of two valid stored normals: their half chord in units of 1 / 16384.
LMX_NV_FN int32_t angle_index(Packed a, Packed b) {
  // |difference of two int16| <= 65535, its square is below 2^32: 32-bit products, a 64-bit sum
  const uint32_t dx = (uint32_t)(comp(a, 0) - comp(b, 0)), dy = (uint32_t)(comp(a, 1) - comp(b, 1)), dz = (uint32_t)(comp(a, 2) - comp(b, 2));
  const uint64_t c2 = (uint64_t)(dx * dx) + (uint64_t)(dy * dy) + (uint64_t)(dz * dz);
  const float c = sqrtf((float)c2);
  const int32_t i = (int32_t)rintf(c * 0.5f);
  return i < kUnit ? i : kUnit;
}

// A crop pixel that counts for the depth term, with the two stored normals that meet there.
LMX_NV_FN void add_met_normals(Packed t, Packed s, const uint32_t* table, Sums* a) {
  if (!valid(t) || !valid(s)) return;
  a->sum_angle_urad += (uint64_t)table[angle_index(t, s)];
  a->n_normal += 1;
}

// dv::add_vector with both terms, as the kernel reads a crop row: word[] as there, tn[e] the stored normal of element col0 + e (the
// padding's normals are zeros, like its depths).  row_in: srow / snrow are the scene row's depths and normals; otherwise neither is read.
// Both scene reads of an element sit under the in-image predicate and nowhere else: the depth where t != 0, the normal where the crop's
// normal is valid (which implies t != 0).  Every load comes before every sum, so neither scene read waits for the other and the chain of
// dependent loads is crop -> scene -> table.
LMX_NV_FN void add_vector(const uint32_t word[4], const Packed tn[dv::kPitchAlign], bool row_in, int32_t x, int32_t col0, int32_t W, const uint16_t* srow,
                          const Packed* snrow, const uint32_t* table, dv::Sums* a, Sums* b) {
  uint16_t t[dv::kPitchAlign], s[dv::kPitchAlign];
  Packed sn[dv::kPitchAlign];
  LMX_NV_UNROLL
  for (int e = 0; e < dv::kPitchAlign; ++e) {
    t[e] = (uint16_t)(word[e >> 1] >> (16 * (e & 1)));
    int32_t X = 0;
    const bool in = row_in && dv::scene_col(x, col0 + e, W, &X);
    s[e] = (in && t[e] != 0) ? srow[X] : (uint16_t)0;
    sn[e] = (in && valid(tn[e])) ? snrow[X] : (Packed)0;
  }
  LMX_NV_UNROLL
  for (int e = 0; e < dv::kPitchAlign; ++e) {
    dv::add_template_pixel(t[e], a);
    dv::add_met_pixel(t[e], s[e], a);
    if (s[e] != 0) add_met_normals(tn[e], sn[e], table, b);     // s != 0 only where the pixel met the scene
  }
}

// One whole match, pixel by pixel, both terms: the definition the kernel is tested against.  crop / crop_normals: [h][pitch]; scene /
// scene_normals: [H] rows of scene_pitch elements.  The depth half is dv::diff_match.
LMX_NV_FN void diff_match(const uint16_t* crop, const Packed* crop_normals, int32_t w, int32_t h, int32_t pitch, const uint16_t* scene,
                          const Packed* scene_normals, int32_t W, int32_t H, size_t scene_pitch, int32_t x, int32_t y, const uint32_t* table, dv::Sums* dd,
                          Sums* nd) {
  dv::Sums a = {0, 0, 0};
  Sums n = {0, 0};
  for (int32_t i = 0; i < h; ++i) {
    int32_t Y = 0;
    const bool row_in = dv::scene_row(y, i, H, &Y);
    for (int32_t j = 0; j < w; ++j) {
      const uint16_t t = crop[(size_t)i * (size_t)pitch + j];
      if (t == 0) continue;
      dv::add_template_pixel(t, &a);
      int32_t X = 0;
      if (!row_in || !dv::scene_col(x, j, W, &X)) continue;
      const uint16_t s = scene[(size_t)Y * scene_pitch + (size_t)X];
      dv::add_met_pixel(t, s, &a);
      if (s != 0) add_met_normals(crop_normals[(size_t)i * (size_t)pitch + j], scene_normals[(size_t)Y * scene_pitch + (size_t)X], table, &n);
    }
  }
  *dd = a;
  *nd = n;
}

// The same match walked the way the kernel walks it: whole vectors over the padded rows (the padding's depths and normals must be zeros).
LMX_NV_FN void diff_match_vectors(const uint16_t* crop, const Packed* crop_normals, int32_t h, int32_t pitch, const uint16_t* scene, const Packed* scene_normals,
                                  int32_t W, int32_t H, size_t scene_pitch, int32_t x, int32_t y, const uint32_t* table, dv::Sums* dd, Sums* nd) {
  dv::Sums a = {0, 0, 0};
  Sums n = {0, 0};
  for (int32_t i = 0; i < h; ++i) {
    int32_t Y = 0;
    const bool row_in = dv::scene_row(y, i, H, &Y);
    for (int32_t c = 0; c < pitch; c += dv::kPitchAlign) {
      const uint16_t* p = crop + (size_t)i * (size_t)pitch + c;
      uint32_t word[4];
      for (int k = 0; k < 4; ++k) word[k] = (uint32_t)p[2 * k] | ((uint32_t)p[2 * k + 1] << 16);
      add_vector(word, crop_normals + (size_t)i * (size_t)pitch + c, row_in, x, c, W, scene + (size_t)Y * scene_pitch, scene_normals + (size_t)Y * scene_pitch,
                 table, &a, &n);
    }
  }
  *dd = a;
  *nd = n;
}

// What a cluster's depth-and-normal score is the mean of (lmx_ctx_collect_clusters_depth_normal, lmx_match_value): minus (the mean absolute
// depth difference in metres + the mean normal angle in radians), or no_value for a match that had nothing to compare in either term.  The
// reference's getClusterScore is 1 / exp(a) * 1 / exp(b) of the two means: exp of this value.
template <typename DDiff, typename NDiff>
LMX_NV_FN double value(const DDiff& d, const NDiff& n, double no_value) {
  if (d.n_valid <= 0 || n.n_normal <= 0) return no_value;
  return -((double)d.sum_abs_mm / ((double)d.n_valid * 1000.0) + (double)n.sum_angle_urad / ((double)n.n_normal * 1e6));
}

// The chord -> angle map, in double on the host (host code only): out[kAngleTableSize].
inline void build_angle_table(uint32_t* out) {
  for (int i = 0; i < kAngleTableSize; ++i) {
    const double h = (double)i / (double)kUnit;
    out[i] = (uint32_t)llrint(2e6 * asin(h < 1.0 ? h : 1.0));
  }
}

}  // namespace nv
}  // namespace lmx
