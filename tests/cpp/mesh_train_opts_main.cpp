// Trains a bank from a mesh through the C++ facade with the options argument (include/lmx_linemod.hpp, Detector::addTemplatesFromMesh with
// lmx_train_mesh_opts: candidates found and compacted on the device) and prints what tests/test_gpu_train_candidates.py compares with the
// Python host path.
//   mesh_train_opts_main <triangles.f64> <views.f64> <width> <height> <focal> <out_templates.yml>
// triangles.f64: n x 9 doubles; views.f64: m x 10 doubles (R row major, distance).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "lmx_linemod.hpp"

static std::vector<double> read_doubles(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(1); }
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<double> out(raw.size() / sizeof(double));
  std::memcpy(out.data(), raw.data(), out.size() * sizeof(double));
  return out;
}

int main(int argc, char** argv) {
  if (argc != 7) { std::fprintf(stderr, "usage: mesh_train_opts_main triangles.f64 views.f64 width height focal out.yml\n"); return 2; }
  try {
    const std::vector<double> tri = read_doubles(argv[1]), vw = read_doubles(argv[2]);
    std::vector<lmx_mesh_view> views(vw.size() / 10);
    std::memcpy(views.data(), vw.data(), views.size() * sizeof(lmx_mesh_view));
    lmx_mesh_camera cam;
    cam.width = std::atoi(argv[3]); cam.height = std::atoi(argv[4]);
    cam.fx = cam.fy = std::atof(argv[5]);
    cam.cx = cam.width / 2.0; cam.cy = cam.height / 2.0;
    cam.light[0] = 0.35; cam.light[1] = -0.45; cam.light[2] = -0.82;
    lmx::linemod::Detector det;
    det.create({lmx_modality_desc{LMX_MOD_COLOR_GRADIENT, 10.0f, 55.0f, 63, 0, 0, 0}, lmx_modality_desc{LMX_MOD_DEPTH_NORMAL, 0.0f, 0.0f, 63, 2000, 50, 2}}, {5, 8});
    lmx_renderer_params* side = nullptr;
    const lmx_train_mesh_opts opts = {(uint32_t)sizeof(lmx_train_mesh_opts), LMX_TRAIN_CANDIDATES_DEVICE};
    lmx_train_mesh_stats stats;
    const std::vector<int> ids = det.addTemplatesFromMesh(tri, cam, views, "obj", &side, &opts, &stats);
    int accepted = 0;
    for (int id : ids) accepted += id >= 0;
    std::printf("views %zu accepted %d templates %d side_car %zu device_views %d fallback_views %d\n", ids.size(), accepted, det.numTemplates("obj"),
                side ? side->n_templates : 0, stats.n_device_views, stats.n_fallback_views);
    lmx_renderer_params_free(side);
    det.write(argv[6]);
  } catch (const lmx::linemod::Exception& e) {
    std::fprintf(stderr, "exception status %d: %s\n", (int)e.status, e.what());
    return 1;
  }
  return 0;
}
