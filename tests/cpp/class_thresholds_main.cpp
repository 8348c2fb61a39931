// A caller of the per-class match thresholds: one bank of several classes matched in one call, every class at its own threshold
// (lmx::linemod::Detector::match with a std::map<std::string, float> in place of `threshold`), the way the reference's two-detector node
// would run as one bank with 92 for one object and 94 for the other.  Prints what tests/test_gpu_class_thresholds.py compares with the
// Python path.
//   class_thresholds_main <bank.yml> <directory> <width> <height> <class> <threshold> [<class> <threshold> ...]
// <directory> holds source_0.bin (BGR, dense rows) and source_1.bin (16-bit depth).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <vector>

#include "lmx_linemod.hpp"

template <typename T>
static std::vector<T> read_file(const std::string& path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(1); }
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> out(raw.size() / sizeof(T));
  std::memcpy(out.data(), raw.data(), out.size() * sizeof(T));
  return out;
}

int main(int argc, char** argv) {
  if (argc < 7 || argc % 2 != 1) { std::fprintf(stderr, "usage: class_thresholds_main bank.yml directory width height class threshold [class threshold ...]\n"); return 2; }
  try {
    const std::string dir = argv[2];
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
    const std::vector<uint8_t> bgr = read_file<uint8_t>(dir + "/source_0.bin");
    const std::vector<uint16_t> depth = read_file<uint16_t>(dir + "/source_1.bin");
    if (bgr.size() != (size_t)W * H * 3 || depth.size() != (size_t)W * H) { std::fprintf(stderr, "the source files do not hold %d x %d pixels\n", W, H); return 2; }
    std::map<std::string, float> thresholds;
    for (int i = 5; i + 1 < argc; i += 2) thresholds[argv[i]] = (float)std::atof(argv[i + 1]);

    lmx::linemod::Detector det;
    det.read(argv[1]);
    const lmx::linemod::Image color{bgr.data(), H, W, 3, 1, (size_t)W * 3};
    const lmx::linemod::Image depth_img{depth.data(), H, W, 1, 2, (size_t)W * 2};
    std::vector<lmx::linemod::Match> matches;
    det.match({color, depth_img}, thresholds, matches);
    std::printf("matches %zu\n", matches.size());
    for (const lmx::linemod::Match& m : matches) std::printf("%d %d %.9g %s %d\n", m.x, m.y, m.similarity, m.class_id.c_str(), m.template_id);
  } catch (const lmx::linemod::Exception& e) {
    std::fprintf(stderr, "exception status %d: %s\n", (int)e.status, e.what());
    return 1;
  }
  return 0;
}
