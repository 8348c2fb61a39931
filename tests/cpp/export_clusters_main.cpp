// A complete caller of the scored way out: frames and depth scene in device memory go in (Detector::uploadDevice,
// DepthTemplates::uploadSceneDevice), the matches, their depth and normal sums and the clusters ranked by both stay in device memory
// (Detector::exportClusters, score 2) for a next stage on the caller's stream -- here a copy back on that stream, with ONE synchronisation.
// The same enqueue then goes through lmx_ctx_collect_clusters_depth_normal, and both results are printed for
// tests/test_gpu_export_clusters_cpp.py to compare.
//   export_clusters_main <templates.yml> <sidecar.f64> <width> <height> <n_frames> <frames_bgr.u8> <frames_depth.u16> <threshold>
//                        <max_large_frames> <crop_sizes.i32> <crops.u16> <focal length>
// sidecar.f64: per template {origin distance, rect x, y, w, h} as doubles; crop_sizes.i32: per template {w, h}; crops.u16: the crops, dense,
// one after the other; the frame files hold n_frames dense frames one after the other.
#include <hip/hip_runtime_api.h>

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

#define HIP_OK(expr)                                                                                          \
  do {                                                                                                        \
    const hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); std::exit(1); }   \
  } while (0)

template <typename T>
static T* device_array(size_t n) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
  return static_cast<T*>(p);
}

static void print_frame(const char* who, int f, const lmx_match_t* m, const lmx_depth_diff_t* d, const lmx_normal_diff_t* nd, size_t nm, const lmx_cluster_t* c,
                        size_t nc, const int32_t* members) {
  std::printf("%s frame %d matches %zu clusters %zu\n", who, f, nm, nc);
  for (size_t i = 0; i < nm; ++i)
    std::printf("%s m %d %d %.9g %d %d depth %lld %d %d normal %lld %d\n", who, m[i].x, m[i].y, m[i].similarity, m[i].template_id, m[i].class_index,
                (long long)d[i].sum_abs_mm, d[i].n_valid, d[i].n_template, (long long)nd[i].sum_angle_urad, nd[i].n_normal);
  for (size_t k = 0; k < nc; ++k) {
    std::printf("%s c %d %d %d rect %d %d %d %d score %.17g members", who, c[k].index[0], c[k].index[1], c[k].index[2], c[k].rect[0], c[k].rect[1], c[k].rect[2],
                c[k].rect[3], c[k].score);
    for (int32_t j = 0; j < c[k].member_count; ++j) std::printf(" %d", members[c[k].member_begin + j]);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc != 13) {
    std::fprintf(stderr, "usage: export_clusters_main templates.yml sidecar.f64 width height n_frames frames_bgr.u8 frames_depth.u16 threshold max_large_frames "
                         "crop_sizes.i32 crops.u16 focal_length\n");
    return 2;
  }
  try {
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), F = std::atoi(argv[5]);
    const std::vector<double> side = read_file<double>(argv[2]);
    const std::vector<uint8_t> bgr = read_file<uint8_t>(argv[6]);
    const std::vector<uint16_t> depth = read_file<uint16_t>(argv[7]);
    const std::vector<int32_t> sizes = read_file<int32_t>(argv[10]);
    const std::vector<uint16_t> crop_data = read_file<uint16_t>(argv[11]);
    const size_t px = (size_t)W * H;
    if (F < 1 || bgr.size() != px * 3 * F || depth.size() != px * F) { std::fprintf(stderr, "the frame files do not hold %d frames of %d x %d\n", F, W, H); return 2; }
    std::shared_ptr<lmx::linemod::Detector> det = lmx::linemod::readLinemod(argv[1]);
    det->setDevice(0, F, 1 << 17);

    // one crop per template, with normals
    std::vector<const uint16_t*> crops;
    std::vector<std::pair<int, int> > wh;
    size_t at = 0;
    for (size_t i = 0; i + 1 < sizes.size(); i += 2) {
      crops.push_back(crop_data.data() + at);
      wh.push_back(std::make_pair((int)sizes[i], (int)sizes[i + 1]));
      at += (size_t)sizes[i] * (size_t)sizes[i + 1];
    }
    if (at != crop_data.size()) { std::fprintf(stderr, "the crop file does not hold the crops the size file lists\n"); return 2; }
    lmx::linemod::DepthTemplates templates;
    templates.fromCrops(crops, wh);
    templates.enableNormals(std::atof(argv[12]), std::atof(argv[12]));

    hipStream_t stream;
    HIP_OK(hipSetDevice(0));
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    uint8_t* d_bgr = device_array<uint8_t>(bgr.size());
    uint16_t* d_depth = device_array<uint16_t>(depth.size());
    HIP_OK(hipMemcpyAsync(d_bgr, bgr.data(), bgr.size(), hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_depth, depth.data(), depth.size() * 2, hipMemcpyHostToDevice, stream));
    std::vector<std::vector<lmx::linemod::Image> > frames;
    std::vector<lmx::linemod::Image> scene;
    for (int f = 0; f < F; ++f) {
      frames.push_back({lmx::linemod::Image{d_bgr + px * 3 * f, H, W, 3, 1, (size_t)W * 3}, lmx::linemod::Image{d_depth + px * f, H, W, 1, 2, (size_t)W * 2}});
      scene.push_back(frames.back()[1]);
    }
    det->uploadDevice(frames, nullptr, stream);

    lmx_ctx* const ctx = det->context();
    const size_t n_templates = side.size() / 5;
    std::vector<double> dists(n_templates);
    std::vector<int32_t> rects(n_templates * 4);
    for (size_t i = 0; i < n_templates; ++i) {
      dists[i] = side[5 * i];
      for (int k = 0; k < 4; ++k) rects[4 * i + k] = (int32_t)side[5 * i + 1 + k];
    }
    lmx_cluster_params pp;
    pp.vote_row_col_step = 10; pp.renderer_radius_min = 0.5; pp.renderer_radius_step = 0.1; pp.cluster_size_thresh = 2;
    lmx::linemod::check(lmx_ctx_set_cluster_sidecar(ctx, dists.data(), rects.data(), n_templates, &pp));
    lmx::linemod::check(lmx_ctx_enqueue(ctx, F, (float)std::atof(argv[8]), nullptr, 0));
    templates.uploadSceneDevice(scene, stream);   // after the enqueue, from the same device frames

    // the results stay on the device, behind `stream`
    const size_t cap = 1 << 15;
    lmx_export_clusters_desc desc;
    std::memset(&desc, 0, sizeof(desc));
    desc.struct_size = sizeof(desc);
    desc.score = 2;
    desc.class_index = -1;
    desc.templates = templates.handle();
    desc.no_value = -HUGE_VAL;
    desc.max_large_frames = std::atoi(argv[9]);
    desc.header = device_array<uint32_t>(16);
    desc.frame_info = device_array<int32_t>((size_t)F * 8);
    desc.matches = device_array<lmx_match_t>(cap); desc.cap_matches = cap;
    desc.diffs = device_array<lmx_depth_diff_t>(cap);
    desc.ndiffs = device_array<lmx_normal_diff_t>(cap);
    desc.clusters_out = device_array<lmx_cluster_t>(cap); desc.cap_clusters = cap;
    desc.members = device_array<int32_t>(cap); desc.cap_members = cap;
    det->exportClusters(desc, stream);
    // "the next stage": here the copy back, on the same stream; the one synchronisation of this program
    uint32_t header[16];
    std::vector<int32_t> info((size_t)F * 8);
    std::vector<lmx_match_t> matches(cap);
    std::vector<lmx_depth_diff_t> diffs(cap);
    std::vector<lmx_normal_diff_t> ndiffs(cap);
    std::vector<lmx_cluster_t> clusters(cap);
    std::vector<int32_t> members(cap);
    HIP_OK(hipMemcpyAsync(header, desc.header, sizeof(header), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(info.data(), desc.frame_info, info.size() * 4, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(matches.data(), desc.matches, cap * sizeof(lmx_match_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(diffs.data(), desc.diffs, cap * sizeof(lmx_depth_diff_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(ndiffs.data(), desc.ndiffs, cap * sizeof(lmx_normal_diff_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(clusters.data(), desc.clusters_out, cap * sizeof(lmx_cluster_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(members.data(), desc.members, cap * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    std::printf("header frames %u flags %u matches %u clusters %u members %u\n", header[0], header[1], header[2], header[3], header[4]);
    for (int f = 0; f < F; ++f) {
      const int32_t* fi = info.data() + (size_t)f * 8;
      std::printf("export frame %d status %d raw_records %d\n", f, fi[6], fi[7]);
      if (fi[6] == 0)
        print_frame("export", f, matches.data() + fi[0], diffs.data() + fi[0], ndiffs.data() + fi[0], (size_t)fi[1], clusters.data() + fi[2], (size_t)fi[3], members.data());
    }

    // the same enqueue through the host path
    std::vector<size_t> mo((size_t)F + 1), co((size_t)F + 1);
    lmx::linemod::check(lmx_ctx_collect_clusters_depth_normal(ctx, F, templates.handle(), -1, -HUGE_VAL, matches.data(), cap, mo.data(), diffs.data(), ndiffs.data(),
                                                              clusters.data(), cap, co.data(), members.data(), cap));
    for (int f = 0; f < F; ++f)
      print_frame("collect", f, matches.data() + mo[f], diffs.data() + mo[f], ndiffs.data() + mo[f], mo[f + 1] - mo[f], clusters.data() + co[f], co[f + 1] - co[f],
                  members.data());

    for (void* p : {(void*)desc.header, (void*)desc.frame_info, (void*)desc.matches, (void*)desc.diffs, (void*)desc.ndiffs, (void*)desc.clusters_out, (void*)desc.members,
                    (void*)d_bgr, (void*)d_depth})
      HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(stream));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
