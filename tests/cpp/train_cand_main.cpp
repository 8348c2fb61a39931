// The candidate lists of the mesh trainer's device path, CPU build, as a stand-alone program for a build with -fsanitize=address,undefined
// (tests/test_train_cand_host.py runs it as a plain child process: the sanitizer's runtime is linked into the program, nothing is
// preloaded).  Runs every level and modality of every case of a file (the format tests/cpp/train_select_main.cpp documents, written by
// train_select_cases.write_cases) through tch_window and tch_select (tests/cpp/train_cand_host.cpp) and prints what it got.
//   train_cand_main <cases.bin>
// Output, per case, level and modality: "<case> <level> <modality> <n_cands> <area> <status>" where status is the feature count or -1
// (rejected), then " F <3 per feature>" if accepted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "train_cand_host.cpp"

namespace {
struct Reader {
  std::vector<char> raw;
  size_t pos = 0;
  void take(void* dst, size_t n) {
    if (pos + n > raw.size()) { std::fprintf(stderr, "cases file ends early\n"); std::exit(2); }
    std::memcpy(dst, raw.data() + pos, n);
    pos += n;
  }
  int32_t i32() { int32_t v; take(&v, 4); return v; }
  float f32() { float v; take(&v, 4); return v; }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: train_cand_main cases.bin\n"); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  Reader rd;
  rd.raw.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int n_cases = rd.i32();
  for (int c = 0; c < n_cases; ++c) {
    const int L = rd.i32(), M = rd.i32();
    if (L < 1 || L > 8 || M < 1 || M > 8) { std::fprintf(stderr, "case %d: %d levels x %d modalities\n", c, L, M); return 2; }
    std::vector<int> is_color(M), nf(M), et(M);
    std::vector<float> strong(M);
    for (int m = 0; m < M; ++m) { is_color[m] = rd.i32(); nf[m] = rd.i32(); strong[m] = rd.f32(); et[m] = rd.i32(); }
    for (int l = 0; l < L; ++l) {
      const int rows = rd.i32(), cols = rd.i32(), has_mask = rd.i32();
      if (rows < 1 || cols < 1 || rows > 4096 || cols > 4096) { std::fprintf(stderr, "case %d: level %d is %d x %d\n", c, l, cols, rows); return 2; }
      const size_t n = (size_t)rows * cols;
      std::vector<std::vector<uint8_t>> lab(M);
      std::vector<std::vector<float>> mag(M);
      std::vector<uint8_t> msk;
      for (int m = 0; m < M; ++m) {
        lab[m].resize(n); rd.take(lab[m].data(), n);
        if (is_color[m]) { mag[m].resize(n); rd.take(mag[m].data(), n * 4); }
      }
      if (has_mask) { msk.resize(n); rd.take(msk.data(), n); }
      for (int m = 0; m < M; ++m) {
        std::vector<uint32_t> records(2 * n + 2), header(16);
        const int nc = tch_window(is_color[m], lab[m].data(), is_color[m] ? mag[m].data() : nullptr, has_mask ? msk.data() : nullptr, rows, cols, strong[m],
                                  et[m] >> l, records.data(), (int)n, header.data());
        if (nc < 0) { std::fprintf(stderr, "case %d level %d modality %d: tch_window returned %d\n", c, l, m, nc); return 2; }
        const int nfl = nf[m] >> l;
        std::vector<int32_t> feats(3 * 64);
        const int st = tch_select(is_color[m], records.data(), header.data(), nfl, feats.data());
        std::printf("%d %d %d %d %u %d", c, l, m, nc, header[1], st);
        if (st > 0) {
          std::printf(" F");
          for (int j = 0; j < 3 * st; ++j) std::printf(" %d", feats[j]);
        }
        std::printf("\n");
      }
    }
  }
  std::printf("train_cand_main ok %d cases\n", n_cases);
  return 0;
}
