// A complete caller of the consumer chain scored by both terms of the reference's depth_normal_diff_calc: trains a small bank from a mesh
// (lmx::linemod::Detector), keeps the templates' depth renders and their normals on the device (DepthTemplates::fromMesh, enableNormals),
// enqueues a scene on a context of its own, hands the scene's depth frame to the templates right behind the enqueue and collects final
// matches, their depth and normal differences and the clusters ranked by lmx_match_value in ONE call
// (lmx_ctx_collect_clusters_depth_normal).  Prints what tests/test_gpu_normal_verify.py compares with the Python path.
//   normal_verify_main <triangles.f64> <views.f64> <width> <height> <focal> <scene_bgr.u8> <scene_depth.u16> <threshold>
// triangles.f64: n x 9 doubles; views.f64: m x 10 doubles (R row major, distance); the scene files are dense rows.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "lmx_linemod.hpp"

template <typename T>
static std::vector<T> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(1); }
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> out(raw.size() / sizeof(T));
  std::memcpy(out.data(), raw.data(), out.size() * sizeof(T));
  return out;
}

int main(int argc, char** argv) {
  if (argc != 9) { std::fprintf(stderr, "usage: normal_verify_main triangles.f64 views.f64 width height focal scene_bgr.u8 scene_depth.u16 threshold\n"); return 2; }
  struct Context {   // destroyed before the detector whose bank it reads
    lmx_ctx* h = nullptr;
    ~Context() { if (h) lmx_ctx_destroy(h); }
  };
  lmx_renderer_params* side = nullptr;
  int rc = 0;
  try {
    const std::vector<double> tri = read_file<double>(argv[1]), vw = read_file<double>(argv[2]);
    std::vector<lmx_mesh_view> views(vw.size() / 10);
    std::memcpy(views.data(), vw.data(), views.size() * sizeof(lmx_mesh_view));
    lmx_mesh_camera cam;
    cam.width = std::atoi(argv[3]); cam.height = std::atoi(argv[4]);
    cam.fx = cam.fy = std::atof(argv[5]);
    cam.cx = cam.width / 2.0; cam.cy = cam.height / 2.0;
    cam.light[0] = 0.35; cam.light[1] = -0.45; cam.light[2] = -0.82;
    const std::vector<uint8_t> bgr = read_file<uint8_t>(argv[6]);
    const std::vector<uint16_t> depth = read_file<uint16_t>(argv[7]);
    const size_t px = (size_t)cam.width * cam.height;
    if (bgr.size() != px * 3 || depth.size() != px) { std::fprintf(stderr, "the scene files do not hold %d x %d pixels\n", cam.width, cam.height); return 2; }

    // train: one template per accepted view, the side-car keeps each one's pose and silhouette rect
    lmx::linemod::Detector det;
    det.create({lmx_modality_desc{LMX_MOD_COLOR_GRADIENT, 10.0f, 55.0f, 63, 0, 0, 0}, lmx_modality_desc{LMX_MOD_DEPTH_NORMAL, 0.0f, 0.0f, 63, 2000, 50, 2}}, {5, 8});
    det.addTemplatesFromMesh(tri, cam, views, "obj", &side);
    const size_t n_templates = side->n_templates;

    // the templates' depth renders, in template order: the view of template i is (side->R[i], side->T[i][2])
    std::vector<lmx_mesh_view> template_views(n_templates);
    for (size_t i = 0; i < n_templates; ++i) {
      std::memcpy(template_views[i].R, side->R + 9 * i, 9 * sizeof(double));
      template_views[i].distance = side->T[3 * i + 2];
    }
    lmx::linemod::DepthTemplates renders;
    renders.fromMesh(tri, cam, template_views);
    renders.enableNormals(cam.fx, cam.fy);
    std::printf("templates %zu depth_templates %d device_bytes %zu\n", n_templates, renders.count(), renders.deviceBytes());

    // a context with the consumer chain's side-car
    lmx_ctx_desc desc;
    std::memset(&desc, 0, sizeof(desc));
    desc.width = cam.width; desc.height = cam.height; desc.max_batch = 1;
    Context context;
    lmx::linemod::check(lmx_ctx_create(det.bank(), &desc, &context.h));
    lmx_ctx* const ctx = context.h;
    lmx_cluster_params pp;
    pp.vote_row_col_step = 10; pp.renderer_radius_min = 0.4; pp.renderer_radius_step = 0.05; pp.cluster_size_thresh = 2;
    lmx::linemod::check(lmx_ctx_set_cluster_sidecar(ctx, side->obj_origin_dists, side->rects, n_templates, &pp));

    // enqueue; the scene's depth frame follows while the match kernels run; one call brings matches, differences and clusters
    const lmx::linemod::Image color{bgr.data(), cam.height, cam.width, 3, 1, (size_t)cam.width * 3};
    const lmx::linemod::Image depth_img{depth.data(), cam.height, cam.width, 1, 2, (size_t)cam.width * 2};
    const lmx_image sources[2] = {color.c(), depth_img.c()};
    lmx::linemod::check(lmx_ctx_upload(ctx, 1, sources, 2));
    lmx::linemod::check(lmx_ctx_enqueue(ctx, 1, (float)std::atof(argv[8]), nullptr, 0));
    renders.uploadScene({depth_img});
    const size_t cap = 1 << 16;
    std::vector<lmx_match_t> matches(cap);
    std::vector<lmx_depth_diff_t> diffs(cap);
    std::vector<lmx_normal_diff_t> ndiffs(cap);
    std::vector<lmx_cluster_t> clusters(cap);
    std::vector<int32_t> members(cap);
    size_t match_offsets[2] = {0, 0}, cluster_offsets[2] = {0, 0};
    lmx::linemod::check(lmx_ctx_collect_clusters_depth_normal(ctx, 1, renders.handle(), -1, -HUGE_VAL, matches.data(), cap, match_offsets, diffs.data(),
                                                              ndiffs.data(), clusters.data(), cap, cluster_offsets, members.data(), cap));
    long long sum = 0, valid = 0, angle = 0, normal = 0;
    for (size_t i = 0; i < match_offsets[1]; ++i) { sum += diffs[i].sum_abs_mm; valid += diffs[i].n_valid; angle += ndiffs[i].sum_angle_urad; normal += ndiffs[i].n_normal; }
    std::printf("matches %zu sum_abs_mm %lld n_valid %lld sum_angle_urad %lld n_normal %lld\n", match_offsets[1], sum, valid, angle, normal);
    if (match_offsets[1]) std::printf("first value %.17g\n", lmx::linemod::DepthTemplates::value(diffs[0], ndiffs[0]));
    for (size_t k = 0; k < cluster_offsets[1]; ++k) {
      const lmx_cluster_t& c = clusters[k];
      std::printf("cluster %d %d %d rect %d %d %d %d members %d score %.17g\n", c.index[0], c.index[1], c.index[2], c.rect[0], c.rect[1], c.rect[2], c.rect[3],
                  c.member_count, c.score);
    }
  } catch (const lmx::linemod::Exception& e) {
    std::fprintf(stderr, "exception status %d: %s\n", (int)e.status, e.what());
    rc = 1;
  }
  if (side) lmx_renderer_params_free(side);
  return rc;
}
