// CPU build of the depth check's shared header (linemod_pose_estimation_amd/csrc/lmx_depth_verify.hpp with LMX_DV_HOST): the functions
// tests/test_depth_verify_host.py calls through ctypes, and a main() that runs the border cases on buffers of exactly the needed size, so
// that a build with -fsanitize=address,undefined sees any read outside the crop or the scene and any overflowing coordinate sum.
#define LMX_DV_HOST
#include "lmx_depth_verify.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

using lmx::dv::Sums;

extern "C" int dv_host_pitch(int w) { return lmx::dv::crop_pitch(w); }

// out = {crop-copy grid, lanes of a wave along a crop row, elements of a vector}: how the kernels spread a crop (tests/second_trip_cases.py)
extern "C" void dv_host_launch_caps(int* out) { out[0] = lmx::dv::kCropCopyGrid; out[1] = lmx::dv::kWalkLanes; out[2] = lmx::dv::kPitchAlign; }

// crop: [h][pitch].  vectors = 0: pixel by pixel over the w columns (the padding is not read); 1: whole vectors over the padded rows, as the
// kernel walks them (the padding must be zeros).  out = {sum_abs_mm, n_valid, n_template}.
extern "C" void dv_host_diff(const uint16_t* crop, int w, int h, int pitch, const uint16_t* scene, int W, int H, size_t scene_pitch, int x, int y,
                             int vectors, long long* out) {
  const Sums a = vectors ? lmx::dv::diff_match_vectors(crop, h, pitch, scene, W, H, scene_pitch, x, y)
                         : lmx::dv::diff_match(crop, w, h, pitch, scene, W, H, scene_pitch, x, y);
  out[0] = (long long)a.sum_abs_mm; out[1] = a.n_valid; out[2] = a.n_template;
}

// A list of matches on one core (scripts/depth_verify_bench.py's host comparison): jobs[k] = {x, y, template}, crops[t] = [hs[t]][pitches[t]].
extern "C" void dv_host_diff_batch(const uint16_t* const* crops, const int* ws, const int* hs, const int* pitches, const uint16_t* scene, int W, int H,
                                   const int* jobs, int n, int vectors, long long* out) {
  for (int k = 0; k < n; ++k) {
    const int t = jobs[3 * k + 2];
    dv_host_diff(crops[t], ws[t], hs[t], pitches[t], scene, W, H, (size_t)W, jobs[3 * k], jobs[3 * k + 1], vectors, out + 3 * k);
  }
}

namespace {
uint32_t rng_state = 12345u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
uint16_t value(int zero_percent) {
  if ((int)(rnd() % 100) < zero_percent) return 0;
  const uint32_t k = rnd() % 10;
  return k == 0 ? (uint16_t)1 : k == 1 ? (uint16_t)65535 : (uint16_t)(1 + rnd() % 65535);
}

// the definition once more, in 64-bit coordinates, with nothing shared with the header
Sums plain(const std::vector<uint16_t>& crop, int w, int h, int pitch, const std::vector<uint16_t>& scene, int W, int H, long long x, long long y) {
  Sums a = {0, 0, 0};
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < w; ++j) {
      const long long t = crop[(size_t)i * pitch + j], X = x + j, Y = y + i;
      if (t == 0) continue;
      a.n_template += 1;
      if (X < 0 || X >= W || Y < 0 || Y >= H) continue;
      const long long s = scene[(size_t)Y * W + X];
      if (s == 0) continue;
      a.n_valid += 1;
      a.sum_abs_mm += (uint64_t)(t > s ? t - s : s - t);
    }
  return a;
}
bool same(const Sums& a, const Sums& b) { return a.sum_abs_mm == b.sum_abs_mm && a.n_valid == b.n_valid && a.n_template == b.n_template; }
}  // namespace

int main() {
  const int W = 96, H = 64;
  std::vector<uint16_t> scene((size_t)W * H);   // exactly the image: a read past a row's end lands in the next row, one past the last row outside
  for (uint16_t& v : scene) v = value(20);
  const int widths[] = {1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 129}, heights[] = {1, 3, 4, 5, 9};
  int checked = 0, counted = 0;
  for (int w : widths)
    for (int h : heights) {
      const int pitch = lmx::dv::crop_pitch(w);
      std::vector<uint16_t> crop((size_t)h * pitch, 0);
      for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) crop[(size_t)i * pitch + j] = value(30);
      const int xs[] = {10, 11, 0, -1, -w / 2 - 1, W - w, W - w + 1, W - 1, W - (w + 1) / 2, W, -w, -w + 1, INT_MAX - 1, INT_MAX, INT_MIN, INT_MIN + 1, INT_MAX - w};
      const int ys[] = {7, 0, -1, -h / 2 - 1, H - h, H - h + 1, H - 1, H, -h, -h + 1, INT_MAX - 1, INT_MAX, INT_MIN, INT_MAX - h};
      for (int x : xs)
        for (int y : ys) {
          const Sums want = plain(crop, w, h, pitch, scene, W, H, x, y);
          const Sums a = lmx::dv::diff_match(crop.data(), w, h, pitch, scene.data(), W, H, (size_t)W, x, y);
          const Sums b = lmx::dv::diff_match_vectors(crop.data(), h, pitch, scene.data(), W, H, (size_t)W, x, y);
          if (!same(a, want) || !same(b, want)) {
            std::fprintf(stderr, "crop %dx%d at (%d, %d): want %llu/%d/%d, pixels %llu/%d/%d, vectors %llu/%d/%d\n", w, h, x, y,
                         (unsigned long long)want.sum_abs_mm, want.n_valid, want.n_template, (unsigned long long)a.sum_abs_mm, a.n_valid, a.n_template,
                         (unsigned long long)b.sum_abs_mm, b.n_valid, b.n_template);
            return 1;
          }
          checked += 1;
          counted += want.n_valid > 0;
        }
    }
  // no wrap at 2^32: 257 x 256 pixels of 65535 over a scene of 1
  {
    const int w = 257, h = 256, pitch = lmx::dv::crop_pitch(w), S = 300;
    std::vector<uint16_t> crop((size_t)h * pitch, 0), big((size_t)S * S, 1);
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j) crop[(size_t)i * pitch + j] = 65535;
    const Sums b = lmx::dv::diff_match_vectors(crop.data(), h, pitch, big.data(), S, S, (size_t)S, 20, 30);
    if (b.sum_abs_mm != 4311612928ull || b.n_valid != 65792 || b.n_template != 65792) { std::fprintf(stderr, "large sum: %llu\n", (unsigned long long)b.sum_abs_mm); return 1; }
  }
  std::printf("depth_verify_host ok: %d placements, %d with counting pixels\n", checked, counted);
  return counted > 0 ? 0 : 1;
}
