// CPU build of the pose verification's shared header (linemod_pose_estimation_amd/csrc/lmx_pose_verify.hpp with LMX_PR_HOST): the functions
// tests/test_pose_verify_host.py and tests/test_gpu_pose_verify.py call through ctypes, and a main() that runs poses which put the model
// at, across and beyond the image's borders on buffers of exactly the needed size, so that a build with -fsanitize=address,undefined sees
// any read outside the crop, the scene or the bitmap and any overflowing integer.  Build with -ffp-contract=off.
#define LMX_PR_HOST
#include "lmx_pose_verify.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

namespace pr = lmx::pr;
namespace pv = lmx::pv;

// v: model fx fy cx cy, scene fx fy cx cy, voxel_mm, roi_margin
static pv::Params params_of(const double* v) { return pv::Params{{v[0], v[1], v[2], v[3]}, {v[4], v[5], v[6], v[7]}, v[8], (int32_t)v[9], 0}; }

extern "C" int pv_host_pitch(int w) { return lmx::dv::crop_pitch(w); }
extern "C" int pv_host_record_bytes() { return (int)sizeof(pv::Record); }
extern "C" int pv_host_max_cells() { return pv::kMaxCells; }

// One job.  pose: R[9] then t_mm[3]; record: sizeof(pv::Record) bytes (zeroed first).  1: the parameters are refused, 2: the pose is.
extern "C" int pv_host_verify(const uint16_t* crop, int w, int h, int pitch, int rect_x, int rect_y, const uint16_t* scene, int W, int H, size_t scene_pitch,
                              const double* pose, const double* v, void* record) {
  const pv::Params P = params_of(v);
  if (pv::check_params(P)) return 1;
  if (pv::check_pose(pose, pose + 9)) return 2;
  pv::Record r;
  std::memset(&r, 0, sizeof(r));
  if (w > 0 && h > 0) {
    std::vector<uint32_t> bitmap((size_t)pv::kBitmapWords);   // exactly the bitmap
    pv::verify_job(P, crop, w, h, pitch, rect_x, rect_y, scene, W, H, scene_pitch, pose, pose + 9, bitmap.data(), &r);
  }
  std::memcpy(record, &r, sizeof(r));
  return 0;
}

// A list of jobs on one core (scripts/pose_verify_bench.py's host comparison): jobs[k] = template, poses[k] = R[9] t_mm[3], rects[t] = {x, y},
// a dense scene of W x H.
extern "C" int pv_host_verify_batch(const uint16_t* const* crops, const int* ws, const int* hs, const int* pitches, const int* rects, const uint16_t* scene, int W, int H,
                                    const int* jobs, const double* poses, int n, const double* v, void* records) {
  for (int k = 0; k < n; ++k) {
    const int t = jobs[k];
    if (pv_host_verify(crops[t], ws[t], hs[t], pitches[t], rects[2 * t], rects[2 * t + 1], scene, W, H, (size_t)W, poses + 12 * (size_t)k, v,
                       static_cast<char*>(records) + (size_t)k * sizeof(pv::Record)))
      return 1;
  }
  return 0;
}

extern "C" void pv_host_keep(const void* records, int n, double thresh, unsigned char* keep) {
  for (int k = 0; k < n; ++k) {
    pv::Record r;
    std::memcpy(&r, static_cast<const char*>(records) + (size_t)k * sizeof(r), sizeof(r));
    keep[k] = pv::keep(r, thresh) ? 1 : 0;
  }
}

namespace {
uint32_t rng_state = 2463534242u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
}  // namespace

int main() {
  const int W = 96, H = 80;
  std::vector<uint16_t> scene((size_t)W * H);   // exactly the image
  for (int Y = 0; Y < H; ++Y)
    for (int X = 0; X < W; ++X) scene[(size_t)Y * W + X] = rnd() % 10 == 0 ? (uint16_t)0 : (uint16_t)(600 + (X + 2 * Y) / 4);
  const int shapes[][2] = {{1, 1}, {17, 1}, {33, 37}, {70, 70}};
  int ran = 0, seen[4] = {0, 0, 0, 0}, occupied = 0;
  for (const auto& wh : shapes) {
    const int w = wh[0], h = wh[1], pitch = lmx::dv::crop_pitch(w);
    std::vector<uint16_t> crop((size_t)h * pitch, 0);
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < w; ++j) crop[(size_t)i * pitch + j] = rnd() % 8 == 0 && w * h > 1 ? (uint16_t)0 : (uint16_t)(600 + (j + 2 * i) / 4);
    const int xs[] = {5, 0, -1, -w / 2, W - w, W - w / 2 - 1, W, -w, 1000, -1000, 131072, -131072};
    const int ys[] = {3, -1, -h / 2, H - h / 2 - 1, H, -h, 131072, -131072};
    // identity; a turn about y; one that sends every point behind the camera; one that throws the points far off
    const double poses[][12] = {{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0},
                                {0.984807753012208, 0, 0.17364817766693, 0, 1, 0, -0.17364817766693, 0, 0.984807753012208, -100, 2.5, 9},
                                {1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0},
                                {2, 2, 2, -2, 2, 2, 2, -2, 2, 1048576, -1048576, 1048576}};
    const double voxels[] = {0.25, 4.0, 64.0};
    const int margins[] = {0, 8, 64};
    for (int x : xs)
      for (int y : ys)
        for (const auto& pose : poses)
          for (int q = 0; q < 3; ++q) {
            const double v[10] = {400.0, 400.0, 48.0, 40.0, 400.0, 400.0, 48.0, 40.0, voxels[q], (double)margins[q]};
            pv::Record r;
            if (pv_host_verify(crop.data(), w, h, pitch, x, y, scene.data(), W, H, (size_t)W, pose, v, &r)) return 2;
            if (r.status < pv::OK || r.status > pv::GRID_TOO_LARGE || r.n_occupied > r.n_tested || r.n_tested > r.n_model) {
              std::fprintf(stderr, "crop %dx%d at (%d, %d): status %d, %d of %d of %d\n", w, h, x, y, r.status, r.n_occupied, r.n_tested, r.n_model);
              return 1;
            }
            ran += 1;
            seen[r.status] += 1;
            occupied += r.n_occupied > 0;
          }
  }
  std::printf("pose_verify_host ok: %d jobs, statuses %d %d %d, %d with occupied voxels\n", ran, seen[pv::OK], seen[pv::EMPTY], seen[pv::GRID_TOO_LARGE], occupied);
  return seen[pv::OK] > 0 && seen[pv::EMPTY] > 0 && seen[pv::GRID_TOO_LARGE] > 0 && occupied > 0 ? 0 : 1;
}
