// CPU build of the normal term's shared header (linemod_pose_estimation_amd/csrc/lmx_normal_verify.hpp with LMX_NV_HOST): the functions
// tests/test_normal_verify_host.py calls through ctypes, and a main() that runs the constructed cases on buffers of exactly the needed
// size, so that a build with -fsanitize=address,undefined sees any read outside an image, a crop or the table and any overflowing sum.
#define LMX_NV_HOST
#include "lmx_normal_verify.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace nv = lmx::nv;
namespace dv = lmx::dv;

extern "C" void nv_host_table(uint32_t* out) { nv::build_angle_table(out); }

// out = {frame-map grid cap, crop-map grid}: the workgroups of the normal-map kernels (tests/second_trip_cases.py)
extern "C" void nv_host_launch_caps(int* out) { out[0] = nv::kFrameMapGridCap; out[1] = nv::kCropMapGrid; }

// img: [h] rows of `pitch` elements; out: [h][w] packed normals (8 bytes each: four int16 {qx, qy, qz, valid})
extern "C" void nv_host_normal_map(const uint16_t* img, int w, int h, size_t pitch, double fx, double fy, int difference_threshold, int distance_threshold,
                                   uint64_t* out) {
  const nv::Params p = {(float)fx, (float)fy, difference_threshold, distance_threshold};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) out[(size_t)y * w + x] = nv::normal_at(img, w, h, pitch, x, y, p);
}

extern "C" int nv_host_angle_index(uint64_t a, uint64_t b) { return nv::angle_index(a, b); }

// out = {sum_abs_mm, n_valid, n_template, sum_angle_urad, n_normal}
extern "C" void nv_host_diff(const uint16_t* crop, const uint64_t* crop_normals, int w, int h, int pitch, const uint16_t* scene, const uint64_t* scene_normals,
                             int W, int H, size_t scene_pitch, int x, int y, const uint32_t* table, long long* out) {
  dv::Sums d;
  nv::Sums n;
  nv::diff_match(crop, crop_normals, w, h, pitch, scene, scene_normals, W, H, scene_pitch, x, y, table, &d, &n);
  out[0] = (long long)d.sum_abs_mm; out[1] = d.n_valid; out[2] = d.n_template; out[3] = (long long)n.sum_angle_urad; out[4] = n.n_normal;
}

// the same match through nv::diff_match_vectors: crop / crop_normals are [h][pitch], pitch a multiple of 8, the padding zeros
extern "C" void nv_host_diff_vectors(const uint16_t* crop, const uint64_t* crop_normals, int h, int pitch, const uint16_t* scene, const uint64_t* scene_normals,
                                     int W, int H, size_t scene_pitch, int x, int y, const uint32_t* table, long long* out) {
  dv::Sums d;
  nv::Sums n;
  nv::diff_match_vectors(crop, crop_normals, h, pitch, scene, scene_normals, W, H, scene_pitch, x, y, table, &d, &n);
  out[0] = (long long)d.sum_abs_mm; out[1] = d.n_valid; out[2] = d.n_template; out[3] = (long long)n.sum_angle_urad; out[4] = n.n_normal;
}

struct DD { long long sum_abs_mm; int n_valid, n_template; };
struct ND { long long sum_angle_urad; int n_normal, reserved; };
extern "C" double nv_host_value(long long sum_abs_mm, int n_valid, long long sum_angle_urad, int n_normal, double no_value) {
  const DD d = {sum_abs_mm, n_valid, 0};
  const ND n = {sum_angle_urad, n_normal, 0};
  return nv::value(d, n, no_value);
}

namespace {
uint32_t rng_state = 777u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Image {
  int w, h;
  std::vector<uint16_t> d;        // exactly w * h
  std::vector<uint64_t> n;
  Image(int w_, int h_) : w(w_), h(h_), d((size_t)w_ * h_), n((size_t)w_ * h_) {}
  void normals(const nv::Params& p) {
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) n[(size_t)y * w + x] = nv::normal_at(d.data(), w, h, (size_t)w, x, y, p);
  }
};

// An image as the device stores a crop: rows padded with zeros to the pitch, exactly h * pitch elements of each kind.
struct Padded {
  int pitch;
  std::vector<uint16_t> d;
  std::vector<uint64_t> n;
  explicit Padded(const Image& im) : pitch(dv::crop_pitch(im.w)), d((size_t)im.h * pitch, 0), n((size_t)im.h * pitch, 0) {
    for (int y = 0; y < im.h; ++y)
      for (int x = 0; x < im.w; ++x) { d[(size_t)y * pitch + x] = im.d[(size_t)y * im.w + x]; n[(size_t)y * pitch + x] = im.n[(size_t)y * im.w + x]; }
  }
};

int fail(const char* what) { std::fprintf(stderr, "normal_verify_host: %s\n", what); return 1; }
}  // namespace

int main() {
  const nv::Params p = {800.0f, 800.0f, 50, 2000};
  std::vector<uint32_t> table(nv::kAngleTableSize);   // exactly the table: an index past 16384 is a read outside
  nv::build_angle_table(table.data());
  if (table[0] != 0 || table[8192] != 1047198u || table[16384] != 3141593u) return fail("table values");
  for (int i = 1; i < nv::kAngleTableSize; ++i)
    if (table[i] < table[i - 1]) return fail("table not monotone");

  // a plane with every tap valid: det = 22500, ddx = 22500 a, ddy = 22500 b, so q is the unit vector of (fx a, fy b, -d)
  {
    Image im(23, 19);
    for (int y = 0; y < im.h; ++y)
      for (int x = 0; x < im.w; ++x) im.d[(size_t)y * im.w + x] = (uint16_t)(700 + 3 * x - 2 * y);
    im.normals(p);
    const uint64_t q = im.n[(size_t)9 * im.w + 11];
    const double d = 700 + 33 - 18, len = std::sqrt(2400.0 * 2400.0 + 1600.0 * 1600.0 + d * d);
    if (!nv::valid(q) || std::abs(nv::comp(q, 0) - 16384.0 * 2400.0 / len) > 1.0 || std::abs(nv::comp(q, 1) + 16384.0 * 1600.0 / len) > 1.0 ||
        std::abs(nv::comp(q, 2) + 16384.0 * d / len) > 1.0)
      return fail("plane normal");
  }
  // images of every size the scene test uses, random surfaces with holes, far pixels and the extremes of uint16: the map, then the image
  // laid over itself everywhere around and across its borders, pixel by pixel and as the kernel walks it (whole vectors over padded rows;
  // 505 and 513 lie on both sides of the 64 vectors a wave's lanes cover in one trip)
  int placements = 0, counted = 0;
  const int widths[] = {1, 5, 6, 11, 12, 64, 65, 70, 505, 513}, heights[] = {1, 6, 11, 13, 37};
  for (int w : widths)
    for (int h : heights) {
      Image im(w, h), other(w, h);
      for (size_t k = 0; k < im.d.size(); ++k) {
        const uint32_t r = rnd() % 100;
        im.d[k] = r < 10 ? 0 : r < 15 ? 65535 : r < 20 ? 2000 : r < 25 ? 1999 : (uint16_t)(800 + rnd() % 120);
        other.d[k] = r < 50 ? im.d[k] : (uint16_t)(rnd() % 2200);
      }
      im.normals(p);
      other.normals(p);
      const Padded padded(im);
      const int xs[] = {0, 1, -1, -w / 2 - 1, w - 1, w, -w, INT_MAX, INT_MIN, INT_MAX - w};
      const int ys[] = {0, 1, -1, h - 1, h, -h, INT_MAX, INT_MIN, INT_MAX - h};
      for (int x : xs)
        for (int y : ys) {
          dv::Sums d, d0;
          nv::Sums n;
          nv::diff_match(im.d.data(), im.n.data(), w, h, w, other.d.data(), other.n.data(), w, h, (size_t)w, x, y, table.data(), &d, &n);
          d0 = dv::diff_match(im.d.data(), w, h, w, other.d.data(), w, h, (size_t)w, x, y);
          if (d.sum_abs_mm != d0.sum_abs_mm || d.n_valid != d0.n_valid || d.n_template != d0.n_template) return fail("depth half differs from dv::diff_match");
          if (n.n_normal > d.n_valid) return fail("n_normal > n_valid");
          dv::Sums dvec;
          nv::Sums nvec;
          nv::diff_match_vectors(padded.d.data(), padded.n.data(), h, padded.pitch, other.d.data(), other.n.data(), w, h, (size_t)w, x, y, table.data(), &dvec, &nvec);
          if (dvec.sum_abs_mm != d.sum_abs_mm || dvec.n_valid != d.n_valid || dvec.n_template != d.n_template || nvec.sum_angle_urad != n.sum_angle_urad ||
              nvec.n_normal != n.n_normal)
            return fail("the vector walk differs from nv::diff_match");
          placements += 1;
          counted += n.n_normal > 0;
        }
      // identical data: every angle is exactly 0
      dv::Sums d;
      nv::Sums n;
      nv::diff_match(im.d.data(), im.n.data(), w, h, w, im.d.data(), im.n.data(), w, h, (size_t)w, 0, 0, table.data(), &d, &n);
      if (n.sum_angle_urad != 0 || d.sum_abs_mm != 0) return fail("identical data");
    }
  // no wrap at 2^32: 64 x 64 pixels of two steep opposed planes
  {
    Image up(64, 64), down(64, 64);
    for (int y = 0; y < 64; ++y)
      for (int x = 0; x < 64; ++x) { up.d[(size_t)y * 64 + x] = (uint16_t)(100 + 9 * x); down.d[(size_t)y * 64 + x] = (uint16_t)(100 + 9 * (63 - x)); }
    up.normals(p);
    down.normals(p);
    dv::Sums d;
    nv::Sums n;
    nv::diff_match(up.d.data(), up.n.data(), 64, 64, 64, down.d.data(), down.n.data(), 64, 64, (size_t)64, 0, 0, table.data(), &d, &n);
    if (n.n_normal != 4096 || n.sum_angle_urad <= (1ull << 32)) return fail("opposed planes");
    std::printf("opposed planes: sum_angle_urad %llu over %d pixels\n", (unsigned long long)n.sum_angle_urad, n.n_normal);
  }
  std::printf("normal_verify_host ok: %d placements, %d with counting pixels\n", placements, counted);
  return counted > 0 ? 0 : 1;
}
