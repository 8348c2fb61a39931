// The ingest kernel of lmx_ctx_upload_device, CPU build, as a stand-alone program for a build with -fsanitize=address,undefined
// (tests/test_ingest_kernel_host.py runs it as a plain child process: the sanitizer's runtime is linked into the program, nothing is
// preloaded).  Runs every launch of a file written by ingest_cases.write_cases through ing_run (tests/cpp/ingest_host.cpp) and compares
// the frames with the expected ones the file carries.
//   ingest_main <cases.bin>
// File: int32 n_cases; per case 12 x int32 {color, src_channels, dst_channels, blur, depth_float, SH, SW, H, W, crop_x, crop_y, n_frames},
// then per frame int32 pitch, int32 offset, SH rows of the source's row bytes, and the expected frame.  Every source image lives in a
// block of its own that ends where the image does -- at the last row's last byte, or, for a base and pitch of 16-byte multiples, at the
// end of the 16-byte granule that holds it (the most the wide path may read) -- so that a read beyond it is reported.
// Output, per case: "<case> wide <frames on the wide path>"; last line "ingest_main ok <n> cases".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "ingest_host.cpp"

namespace {
struct Reader {
  std::vector<char> raw;
  size_t pos = 0;
  void take(void* dst, size_t n) {
    if (pos + n > raw.size()) { std::fprintf(stderr, "cases file ends early\n"); std::exit(2); }
    if (n) std::memcpy(dst, raw.data() + pos, n);
    pos += n;
  }
  int32_t i32() { int32_t v; take(&v, 4); return v; }
};
uint8_t* block(size_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 64, n ? n : 1) != 0) { std::fprintf(stderr, "out of memory\n"); std::exit(2); }
  return static_cast<uint8_t*>(p);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: ingest_main cases.bin\n"); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  Reader rd;
  rd.raw.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int n_cases = rd.i32();
  for (int c = 0; c < n_cases; ++c) {
    int32_t p[12];
    for (int32_t& v : p) v = rd.i32();
    const int color = p[0], sc = p[1], dc = p[2], blur = p[3], dfloat = p[4], SH = p[5], SW = p[6], H = p[7], W = p[8], cx = p[9], cy = p[10], nf = p[11];
    if (SH < 1 || SW < 1 || SH > 4096 || SW > 4096 || nf < 1 || nf > 64) { std::fprintf(stderr, "case %d: bad shape\n", c); return 2; }
    const size_t src_row = (size_t)SW * (size_t)(color ? sc : (dfloat ? 4 : 2));
    const size_t frame_bytes = ing_frame_bytes(color, sc, dc, dfloat, H, W);
    const size_t out_row = frame_bytes / (size_t)H;
    std::vector<uint8_t*> blocks;
    std::vector<uint64_t> src, stride;
    std::vector<uint8_t> want(frame_bytes * nf);
    for (int k = 0; k < nf; ++k) {
      const int32_t pitch = rd.i32(), offset = rd.i32();
      if (pitch < (int64_t)src_row || offset < 0 || offset > 64) { std::fprintf(stderr, "case %d frame %d: pitch %d offset %d\n", c, k, pitch, offset); return 2; }
      const bool granules = offset % 16 == 0 && pitch % 16 == 0 && (out_row / (color && sc == 1 && dc == 3 ? 3 : 1)) % 16 == 0;
      const size_t tail = granules ? (src_row + 15) / 16 * 16 : src_row;
      uint8_t* b = block((size_t)offset + (size_t)(SH - 1) * pitch + tail);
      blocks.push_back(b);
      for (int y = 0; y < SH; ++y) rd.take(b + offset + (size_t)y * pitch, src_row);
      rd.take(want.data() + frame_bytes * k, frame_bytes);
      src.push_back((uint64_t)(uintptr_t)(b + offset));
      stride.push_back((uint64_t)pitch);
    }
    uint8_t* dst = block(frame_bytes * nf);
    const int wide = ing_run(color, sc, dc, blur, dfloat, SH, SW, H, W, cx, cy, nf, src.data(), stride.data(), dst);
    if (wide < 0) { std::fprintf(stderr, "case %d: ing_run refused it\n", c); return 2; }
    for (size_t i = 0; i < want.size(); ++i)
      if (dst[i] != want[i]) {
        std::fprintf(stderr, "case %d: frame %zu row %zu byte %zu is %d, expected %d\n", c, i / frame_bytes, i % frame_bytes / out_row, i % out_row, dst[i], want[i]);
        return 1;
      }
    std::printf("%d wide %d\n", c, wide);
    std::free(dst);
    for (uint8_t* b : blocks) std::free(b);
  }
  std::printf("ingest_main ok %d cases\n", n_cases);
  return 0;
}
