// A complete caller of the per-class consumer chain: the reference's two-detector node as ONE bank of two classes.  Reads the bank
// (lmx::linemod::Detector::read), gives each class its renderer-params side-car and clustering parameters (setClusterSidecar(class, ...)),
// and gets one frame's matches and per-object clusters from one enqueue and one collect (collectClustersClasses).  Prints what
// tests/test_gpu_cluster_classes.py compares with the Python path.
//   cluster_classes_main <bank.yml> <directory> <width> <height> <threshold>
// <directory> holds source_0.bin (BGR, dense rows), source_1.bin (16-bit depth) and sidecars.txt: the number of classes, then per class
// "n_templates step radius_min radius_step size_thresh", n_templates origin distances, n_templates x 4 rect values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
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
  if (argc != 6) { std::fprintf(stderr, "usage: cluster_classes_main bank.yml directory width height threshold\n"); return 2; }
  try {
    const std::string dir = argv[2];
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
    const std::vector<uint8_t> bgr = read_file<uint8_t>(dir + "/source_0.bin");
    const std::vector<uint16_t> depth = read_file<uint16_t>(dir + "/source_1.bin");
    if (bgr.size() != (size_t)W * H * 3 || depth.size() != (size_t)W * H) { std::fprintf(stderr, "the source files do not hold %d x %d pixels\n", W, H); return 2; }

    lmx::linemod::Detector det;
    det.read(argv[1]);
    std::ifstream sc((dir + "/sidecars.txt").c_str());
    int n_classes = 0;
    sc >> n_classes;
    if (!sc || n_classes != det.numClasses()) { std::fprintf(stderr, "sidecars.txt does not describe the bank's %d classes\n", det.numClasses()); return 2; }
    for (int c = 0; c < n_classes; ++c) {
      size_t n = 0;
      lmx_cluster_params pp;
      sc >> n >> pp.vote_row_col_step >> pp.renderer_radius_min >> pp.renderer_radius_step >> pp.cluster_size_thresh;
      std::vector<double> dists(n);
      std::vector<int32_t> rects(4 * n);
      for (double& v : dists) sc >> v;
      for (int32_t& v : rects) sc >> v;
      if (!sc) { std::fprintf(stderr, "sidecars.txt: class %d is incomplete\n", c); return 2; }
      det.setClusterSidecar(c, dists, rects, pp);
    }

    const lmx::linemod::Image color{bgr.data(), H, W, 3, 1, (size_t)W * 3};
    const lmx::linemod::Image depth_img{depth.data(), H, W, 1, 2, (size_t)W * 2};
    const lmx::linemod::ClassClusters r = det.collectClustersClasses({{color, depth_img}}, (float)std::atof(argv[5]));
    std::printf("matches %zu clusters %zu\n", r.matches.size(), r.clusters.size());
    for (size_t k = 0; k < r.clusters.size(); ++k) {
      const lmx_cluster_t& c = r.clusters[k];
      std::printf("class %d index %d %d %d rect %d %d %d %d score %.17g members", r.cluster_class[k], c.index[0], c.index[1], c.index[2], c.rect[0], c.rect[1],
                  c.rect[2], c.rect[3], c.score);
      for (int32_t j = 0; j < c.member_count; ++j) std::printf(" %d", r.members[(size_t)(c.member_begin + j)]);
      std::printf("\n");
    }
  } catch (const lmx::linemod::Exception& e) {
    std::fprintf(stderr, "exception status %d: %s\n", (int)e.status, e.what());
    return 1;
  }
  return 0;
}
