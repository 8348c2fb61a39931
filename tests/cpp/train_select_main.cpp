// The trainer's host half as a stand-alone program, for a build with -fsanitize=address,undefined (tests/test_train_select_host.py runs it as a
// plain child process: the sanitizer's runtime is linked into the program, nothing is preloaded).  Runs every case of a file through
// tsh_pyramid (tests/cpp/train_select_host.cpp) both ways -- whole frames, and select_pyramid with its window rule -- and prints what it got;
// the test compares the lines with the oracle's answers.
//   train_select_main <cases.bin>
// cases.bin, int32 little endian unless said otherwise: n_cases, then per case
//   L M, per modality {is_color num_features strong_threshold(float32) extract_threshold},
//   per level {rows cols has_mask, per modality: rows*cols label bytes [+ rows*cols float32 magnitudes if is_color], rows*cols mask bytes if has_mask}
// Output, per case and mode: "<case> <mode> <status>" and, if accepted, " bb x y w h T <5 per template> F <3 per feature>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "train_select_host.cpp"

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
  if (argc != 2) { std::fprintf(stderr, "usage: train_select_main cases.bin\n"); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  Reader rd;
  rd.raw.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int n_cases = rd.i32();
  for (int c = 0; c < n_cases; ++c) {
    const int L = rd.i32(), M = rd.i32();
    if (L < 1 || L > 8 || M < 1 || M > 8) { std::fprintf(stderr, "case %d: %d levels x %d modalities\n", c, L, M); return 2; }
    std::vector<int> is_color(M), nf(M), et(M), rows(L), cols(L);
    std::vector<float> strong(M);
    for (int m = 0; m < M; ++m) { is_color[m] = rd.i32(); nf[m] = rd.i32(); strong[m] = rd.f32(); et[m] = rd.i32(); }
    std::vector<std::vector<uint8_t>> lab((size_t)L * M), msk(L);
    std::vector<std::vector<float>> mag((size_t)L * M);
    std::vector<const void*> lab_p((size_t)L * M), mag_p((size_t)L * M, nullptr), msk_p(L, nullptr);
    size_t total = 0;
    for (int l = 0; l < L; ++l) {
      rows[l] = rd.i32(); cols[l] = rd.i32();
      const int has_mask = rd.i32();
      if (rows[l] < 1 || cols[l] < 1 || rows[l] > 4096 || cols[l] > 4096) { std::fprintf(stderr, "case %d: level %d is %d x %d\n", c, l, cols[l], rows[l]); return 2; }
      const size_t n = (size_t)rows[l] * cols[l];
      for (int m = 0; m < M; ++m) {
        const size_t k = (size_t)l * M + m;
        lab[k].resize(n); rd.take(lab[k].data(), n); lab_p[k] = lab[k].data();
        if (is_color[m]) { mag[k].resize(n); rd.take(mag[k].data(), n * 4); mag_p[k] = mag[k].data(); }
      }
      if (has_mask) { msk[l].resize(n); rd.take(msk[l].data(), n); msk_p[l] = msk[l].data(); }
    }
    for (int m = 0; m < M; ++m) total += (size_t)(nf[m] > 0 ? nf[m] : 0) * L;
    for (int mode = 0; mode < 2; ++mode) {
      std::vector<int32_t> templates((size_t)L * M * 5), features(3 * total + 3);
      int32_t bb[4];
      char err[256];
      const int st = tsh_pyramid(mode, L, M, is_color.data(), rows.data(), cols.data(), nullptr, nullptr, lab_p.data(), mag_p.data(), msk_p.data(), nf.data(),
                                 strong.data(), et.data(), templates.data(), features.data(), bb, err, (int)sizeof(err));
      std::printf("%d %d %d", c, mode, st);
      if (st == 0) {
        std::printf(" bb %d %d %d %d T", bb[0], bb[1], bb[2], bb[3]);
        int n_feat = 0;
        for (int k = 0; k < L * M; ++k) { for (int j = 0; j < 5; ++j) std::printf(" %d", templates[(size_t)k * 5 + j]); n_feat += templates[(size_t)k * 5 + 4]; }
        std::printf(" F");
        for (int j = 0; j < 3 * n_feat; ++j) std::printf(" %d", features[j]);
      }
      std::printf("\n");
    }
  }
  std::printf("train_select_main ok %d cases\n", n_cases);
  return 0;
}
