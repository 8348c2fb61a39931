// The colour quantiser's one-plane instantiation (color_quantize_tile<TH, TRAIN, 1>: the gray context's path, LMX_CTX_GRAY) compiled for the
// CPU like tests/cpp/cq_host.cpp: LMX_CQ_HOST swaps the few machine instructions for plain C++ and the 256 threads of a workgroup run as a loop
// inside every stage.  tests/test_gray_color_kernel_host.py compares its label images, one-byte pyrDown and magnitudes with the oracle run on
// the gray image copied into B, G and R.  Test infrastructure: not part of liblmx.so.
#define LMX_CQ_HOST 1
#include "lmx_color_quantize.hpp"

namespace {
struct HostRun {
  template <typename F>
  void operator()(F&& stage) const {
    for (int tid = 0; tid < 256; ++tid) stage(tid);
  }
};

template <int TH, bool TRAIN>
void run_image(const uint8_t* src, uint8_t* dst, uint8_t* pyr, float* mag, int H, int W, float thr_sq) {
  static uint8_t lds[lmx::cq::Geo<TH, 1>::LDS_BYTES + 64];
  const int tx = (W + lmx::cq::TW - 1) / lmx::cq::TW, ty = (H + TH - 1) / TH;
  for (int y = 0; y < ty; ++y)
    for (int x = 0; x < tx; ++x) {
      for (size_t i = 0; i < sizeof(lds); ++i) lds[i] = (uint8_t)(0xa5 ^ i);   // whatever the previous workgroup left behind
      lmx::cq::color_quantize_tile<TH, TRAIN, 1>(x, y, src, dst, pyr, mag, H, W, thr_sq, lds, HostRun{});
    }
}
}  // namespace

extern "C" {
// src: gray u8 [H][W]; dst: labels u8 [H][W]; pyr: u8 [H/2][W/2] or null; mag: float [H][W] or null (the trainer's squared magnitudes)
int cq_host_gray_run(const uint8_t* src, uint8_t* dst, uint8_t* pyr, float* mag, int H, int W, float weak_threshold, int tile_height) {
  const float thr_sq = weak_threshold * weak_threshold;
  if (tile_height == 16) {
    if (mag) run_image<16, true>(src, dst, pyr, mag, H, W, thr_sq);
    else run_image<16, false>(src, dst, pyr, mag, H, W, thr_sq);
  } else if (tile_height == 32) {
    if (mag) run_image<32, true>(src, dst, pyr, mag, H, W, thr_sq);
    else run_image<32, false>(src, dst, pyr, mag, H, W, thr_sq);
  } else {
    return 1;
  }
  return 0;
}
int cq_host_gray_lds_bytes(int tile_height) { return tile_height == 16 ? (int)lmx::cq::Geo<16, 1>::LDS_BYTES : (int)lmx::cq::Geo<32, 1>::LDS_BYTES; }
}
