// Depth check of a match against the rendered depth of its template (lmx_depth_diff_matches, include/lmx.h): the arithmetic of one pixel,
// one row and one match, shared by the HIP kernels (lmx_verify.hip, k_walk and k_walk_records_dev; lmx_f2.hip for value()) and --
// compiled with LMX_DV_HOST -- by plain CPU builds (tests/cpp/depth_verify_host.cpp, tests/cpp/depth_value_host.cpp).
// The reference's form is depth_normal_diff_calc (src/rgbdDetector.cpp:147-282), the depth half.
//
// A template crop t[h][w] and a scene depth image s[H][W], both uint16 millimetres; 0 = "not on the object" in the crop, "no measurement"
// in the scene.  The crop's top-left corner lies at the match position (x, y), any int32:
//
//   crop pixel (i, j) meets scene pixel (X, Y) = (x + j, y + i)      (64-bit sums: no int32 pair overflows)
//   it COUNTS iff t[i][j] != 0, 0 <= X < W, 0 <= Y < H and s[Y][X] != 0
//   n_template = #{t != 0},  n_valid = #{counting},  sum_abs_mm = sum over counting pixels of |int32(t) - int32(s)|, in 64 bits
//
// Crops are stored with their rows padded WITH ZEROS to a pitch of kPitchAlign elements (16 bytes), so a row can be read as whole aligned
// vectors: a padding element has t == 0 and counts nowhere.  The scene has no padding anyone may rely on: a scene element is read only
// under the in-image predicate (scene_col / scene_row).
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef LMX_DV_HOST
#define LMX_DV_FN inline
#else
#define LMX_DV_FN __host__ __device__ __forceinline__
#endif

namespace lmx {
namespace dv {

constexpr int kPitchAlign = 8;      // elements: 16 bytes, one uint4 load
constexpr int kMaxCropSide = 16384; // so that h * pitch and n_template (<= 2^28) fit an int32
// How lmx_verify.hip spreads the work (no part of the definition; the tests size their crops by them): the lanes of a wave that share a
// crop row, each taking the vectors v0, v0 + kWalkLanes, .. of it; the workgroups of 256 lanes that copy one rendered view's crop, a
// vector per lane and trip.
constexpr int kWalkLanes = 64;      // one wave
constexpr int kCropCopyGrid = 16;

struct Sums {
  uint64_t sum_abs_mm;   // <= 2^28 pixels x 65535 < 2^44
  int32_t n_valid;
  int32_t n_template;
};

LMX_DV_FN int32_t crop_pitch(int32_t w) { return (w + (kPitchAlign - 1)) & ~(kPitchAlign - 1); }

// Scene column of crop column j for a match at x: true and *X when it lies inside [0, W).
LMX_DV_FN bool scene_col(int32_t x, int32_t j, int32_t W, int32_t* X) {
  const int64_t v = (int64_t)x + (int64_t)j;
  if (v < 0 || v >= (int64_t)W) return false;
  *X = (int32_t)v;
  return true;
}
// The same for crop row i of a match at y.
LMX_DV_FN bool scene_row(int32_t y, int32_t i, int32_t H, int32_t* Y) {
  const int64_t v = (int64_t)y + (int64_t)i;
  if (v < 0 || v >= (int64_t)H) return false;
  *Y = (int32_t)v;
  return true;
}

LMX_DV_FN void add_template_pixel(uint16_t t, Sums* a) { a->n_template += t != 0; }

// A crop pixel t != 0 that met the scene value s inside the image.
LMX_DV_FN void add_met_pixel(uint16_t t, uint16_t s, Sums* a) {
  if (s == 0) return;
  const int32_t d = (int32_t)t - (int32_t)s;
  a->sum_abs_mm += (uint64_t)(d < 0 ? -d : d);
  a->n_valid += 1;
}

// One aligned vector of a crop row, as the kernel reads it: word[k] holds elements col0 + 2k (low half) and col0 + 2k + 1 of the row, elements
// past the crop's width are the zero padding.  row_in: the row lies inside the scene and srow is that scene row; otherwise srow is not read.
LMX_DV_FN void add_vector(const uint32_t word[4], bool row_in, int32_t x, int32_t col0, int32_t W, const uint16_t* srow, Sums* a) {
  uint16_t t[kPitchAlign], s[kPitchAlign];
  for (int e = 0; e < kPitchAlign; ++e) {   // the loads first, the sums after them
    t[e] = (uint16_t)(word[e >> 1] >> (16 * (e & 1)));
    int32_t X = 0;
    const bool met = t[e] != 0 && row_in && scene_col(x, col0 + e, W, &X);
    s[e] = met ? srow[X] : (uint16_t)0;       // the only scene read, under the in-image predicate; 0 counts nowhere
  }
  for (int e = 0; e < kPitchAlign; ++e) {
    add_template_pixel(t[e], a);
    add_met_pixel(t[e], s[e], a);
  }
}

// One whole match, pixel by pixel: the definition the kernel is tested against.  crop: [h][pitch] (elements past w are never read here);
// scene: [H] rows of scene_pitch elements.
LMX_DV_FN Sums diff_match(const uint16_t* crop, int32_t w, int32_t h, int32_t pitch, const uint16_t* scene, int32_t W, int32_t H, size_t scene_pitch,
                          int32_t x, int32_t y) {
  Sums a = {0, 0, 0};
  for (int32_t i = 0; i < h; ++i) {
    int32_t Y = 0;
    const bool row_in = scene_row(y, i, H, &Y);
    const uint16_t* trow = crop + (size_t)i * (size_t)pitch;
    for (int32_t j = 0; j < w; ++j) {
      const uint16_t t = trow[j];
      if (t == 0) continue;
      add_template_pixel(t, &a);
      int32_t X = 0;
      if (row_in && scene_col(x, j, W, &X)) add_met_pixel(t, scene[(size_t)Y * scene_pitch + (size_t)X], &a);
    }
  }
  return a;
}

// The same match walked the way the kernel walks it: whole vectors over the padded rows (the padding must be zeros).
LMX_DV_FN Sums diff_match_vectors(const uint16_t* crop, int32_t h, int32_t pitch, const uint16_t* scene, int32_t W, int32_t H, size_t scene_pitch, int32_t x,
                                  int32_t y) {
  Sums a = {0, 0, 0};
  for (int32_t i = 0; i < h; ++i) {
    int32_t Y = 0;
    const bool row_in = scene_row(y, i, H, &Y);
    const uint16_t* srow = scene + (size_t)Y * scene_pitch;
    for (int32_t c = 0; c < pitch; c += kPitchAlign) {
      const uint16_t* p = crop + (size_t)i * (size_t)pitch + c;
      uint32_t word[4];
      for (int k = 0; k < 4; ++k) word[k] = (uint32_t)p[2 * k] | ((uint32_t)p[2 * k + 1] << 16);
      add_vector(word, row_in, x, c, W, srow, &a);
    }
  }
  return a;
}

// What a cluster's depth score is the mean of (lmx_cluster_matches_scored, the scored form of k_f2_finalize_cluster): minus the mean absolute
// difference in metres, or no_value for a match that had nothing to compare.  Diff: lmx_depth_diff_t or anything with its fields.
template <typename Diff>
LMX_DV_FN double value(const Diff& d, double no_value) {
  return d.n_valid > 0 ? -((double)d.sum_abs_mm / ((double)d.n_valid * 1000.0)) : no_value;
}

}  // namespace dv
}  // namespace lmx
