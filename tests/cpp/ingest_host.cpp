// The ingest kernel of lmx_ctx_upload_device on the CPU (linemod_pose_estimation_amd/csrc/lmx_ingest.hpp: the header k_ingest is written
// with, compiled here without HIP), behind a C interface.  Compiled with g++ by tests/test_ingest_kernel_host.py and, under
// -fsanitize=address,undefined, into tests/cpp/ingest_main.cpp.
//   ing_run : one launch -- n_frames source images {address, row stride} of one modality -> the frames, packed, at `dst` (16-byte aligned)
#include <cstdint>

#include "lmx_ingest.hpp"

namespace ing = lmx::ingest;

extern "C" {

// -> the number of frames that took the wide path, or -1 for arguments the library would have refused
int ing_run(int color, int src_channels, int dst_channels, int blur, int depth_float, int SH, int SW, int H, int W, int crop_x, int crop_y, int n_frames,
            const uint64_t* src, const uint64_t* row_stride, uint8_t* dst) {
  if (crop_x < 0 || crop_y < 0 || crop_x + W > SW || crop_y + H > SH || W < 1 || H < 1 || n_frames < 1 || n_frames > 64) return -1;
  if (((uintptr_t)dst & 15u) != 0) return -1;
  ing::Args a{};
  const int mode = ing::plan(&a, color != 0, src_channels, dst_channels, blur != 0, depth_float != 0, SH, SW, H, W, crop_x, crop_y);
  a.dst = dst;
  ing::Entry tab[64];
  int wide = 0;
  for (int f = 0; f < n_frames; ++f) {
    tab[f] = ing::Entry{src[f], row_stride[f]};
    wide += ing::is_wide(a, tab[f]) ? 1 : 0;
  }
  ing::run(mode, a, tab, n_frames);
  return wide;
}

// bytes of one output frame of such a launch
uint64_t ing_frame_bytes(int color, int src_channels, int dst_channels, int depth_float, int H, int W) {
  ing::Args a{};
  ing::plan(&a, color != 0, src_channels, dst_channels, false, depth_float != 0, H, W, H, W, 0, 0);
  return a.dst_frame_bytes;
}

}  // extern "C"
