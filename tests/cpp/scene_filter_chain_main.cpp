// A complete caller of the pose chain behind the scene's depth outlier filter, through the C++ facade (include/lmx_linemod.hpp): as
// tests/cpp/pose_chain_main.cpp it trains a small bank from a mesh, keeps the templates' depth renders on the device and stays on the device
// from the frame to the verified poses -- Detector::uploadDevice, the enqueue, DepthTemplates::uploadSceneDevice, Detector::exportClusters
// (the depth score, on the raw scene) and DepthTemplates::poseChain on one stream with nothing read on the host in between -- but with
// DepthTemplates::setSceneFilter in front: the filtered copy of the scene is made on the device inside poseChain, and both pose stages read
// it.  The reference's statisticalOutlierRemoval in front of icpPoseRefine and hypothesisVerification (src/rgbdDetector.cpp:836).  Device
// memory is read back only to print what tests/test_gpu_scene_filter.py compares with the Python path.
//   scene_filter_chain_main <triangles.f64> <views.f64> <width> <height> <focal> <scene_bgr.u8> <scene_depth.u16> <threshold> <collision_rate_threshold>
// triangles.f64: n x 9 doubles; views.f64: m x 10 doubles (R row major, distance); the scene files are dense rows.
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

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: scene_filter_chain_main triangles.f64 views.f64 width height focal scene_bgr.u8 scene_depth.u16 threshold collision_rate_threshold\n");
    return 2;
  }
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

    lmx::linemod::Detector det;
    det.create({lmx_modality_desc{LMX_MOD_COLOR_GRADIENT, 10.0f, 55.0f, 63, 0, 0, 0}, lmx_modality_desc{LMX_MOD_DEPTH_NORMAL, 0.0f, 0.0f, 63, 2000, 50, 2}}, {5, 8});
    lmx_renderer_params* side = nullptr;
    det.addTemplatesFromMesh(tri, cam, views, "obj", &side);
    const size_t n_templates = side->n_templates;
    std::vector<lmx_mesh_view> template_views(n_templates);
    for (size_t i = 0; i < n_templates; ++i) {
      std::memcpy(template_views[i].R, side->R + 9 * i, 9 * sizeof(double));
      template_views[i].distance = side->T[3 * i + 2];
    }
    lmx::linemod::DepthTemplates renders;
    renders.fromMesh(tri, cam, template_views);
    lmx_scene_filter_params fp = lmx::linemod::DepthTemplates::sceneFilterDefaults();   // radius 3, k 15, stddev_mul 1.0
    fp.fx = cam.fx; fp.fy = cam.fy; fp.cx = cam.cx; fp.cy = cam.cy;
    renders.setSceneFilter(&fp);

    // the frame goes to the device once; everything after it is queued on `stream`
    hipStream_t stream;
    HIP_OK(hipSetDevice(0));
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    uint8_t* d_bgr = device_array<uint8_t>(bgr.size());
    uint16_t* d_depth = device_array<uint16_t>(depth.size());
    HIP_OK(hipMemcpyAsync(d_bgr, bgr.data(), bgr.size(), hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_depth, depth.data(), depth.size() * 2, hipMemcpyHostToDevice, stream));
    const lmx::linemod::Image color{d_bgr, cam.height, cam.width, 3, 1, (size_t)cam.width * 3};
    const lmx::linemod::Image depth_img{d_depth, cam.height, cam.width, 1, 2, (size_t)cam.width * 2};
    det.setDevice(0, 1, 1 << 17);
    det.uploadDevice({{color, depth_img}}, nullptr, stream);
    lmx_ctx* const ctx = det.context();
    lmx_cluster_params pp;
    pp.vote_row_col_step = 10; pp.renderer_radius_min = 0.4; pp.renderer_radius_step = 0.05; pp.cluster_size_thresh = 2;
    lmx::linemod::check(lmx_ctx_set_cluster_sidecar(ctx, side->obj_origin_dists, side->rects, n_templates, &pp));
    lmx::linemod::check(lmx_ctx_enqueue(ctx, 1, (float)std::atof(argv[8]), nullptr, 0));
    renders.uploadSceneDevice({depth_img}, stream);   // after the enqueue, from the same device frame

    const size_t cap = 1 << 14, cap_clusters = 1024;
    lmx_export_clusters_desc xd;
    std::memset(&xd, 0, sizeof(xd));
    xd.struct_size = sizeof(xd);
    xd.score = 1;
    xd.class_index = -1;
    xd.templates = renders.handle();
    xd.no_value = -HUGE_VAL;
    xd.max_large_frames = 1;
    xd.header = device_array<uint32_t>(16);
    xd.frame_info = device_array<int32_t>(8);
    xd.matches = device_array<lmx_match_t>(cap); xd.cap_matches = cap;
    xd.diffs = device_array<lmx_depth_diff_t>(cap);
    xd.clusters_out = device_array<lmx_cluster_t>(cap_clusters); xd.cap_clusters = cap_clusters;
    xd.members = device_array<int32_t>(cap); xd.cap_members = cap;
    det.exportClusters(xd, stream);

    // the clusters never leave the device: their leaders, poses, checks and keep decisions are written behind the export
    lmx_pose_refine_params rp = lmx::linemod::DepthTemplates::poseRefineDefaults();
    rp.model_fx = rp.scene_fx = cam.fx; rp.model_fy = rp.scene_fy = cam.fy;
    rp.model_cx = rp.scene_cx = cam.cx; rp.model_cy = rp.scene_cy = cam.cy;
    lmx_pose_verify_params vp = lmx::linemod::DepthTemplates::poseVerifyDefaults();
    vp.model_fx = vp.scene_fx = cam.fx; vp.model_fy = vp.scene_fy = cam.fy;
    vp.model_cx = vp.scene_cx = cam.cx; vp.model_cy = vp.scene_cy = cam.cy;
    lmx_pose_chain_desc cd;
    std::memset(&cd, 0, sizeof(cd));
    cd.class_index = -1;
    cd.refine = &rp; cd.verify = &vp;
    cd.keep_thresh = std::atof(argv[9]);
    cd.header = xd.header; cd.frame_info = xd.frame_info;
    cd.matches = xd.matches; cd.cap_matches = cap;
    cd.clusters = xd.clusters_out; cd.cap_clusters = cap_clusters;
    cd.members = xd.members; cd.cap_members = cap;
    cd.chain_header = device_array<uint32_t>(8);
    cd.leaders = device_array<int32_t>(cap_clusters);
    cd.poses = device_array<lmx_pose_refine_t>(cap_clusters);
    cd.checks = device_array<lmx_pose_verify_t>(cap_clusters);
    cd.keep = device_array<uint8_t>(cap_clusters);
    renders.poseChain(cd, stream);

    // only to print: the copies back on the same stream, and the one synchronisation of this program
    uint32_t header[16], chain[8];
    int32_t info[8];
    std::vector<lmx_match_t> matches(cap);
    std::vector<int32_t> leaders(cap_clusters);
    std::vector<lmx_pose_refine_t> poses(cap_clusters);
    std::vector<lmx_pose_verify_t> checks(cap_clusters);
    std::vector<uint8_t> keep(cap_clusters);
    HIP_OK(hipMemcpyAsync(header, xd.header, sizeof(header), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(info, xd.frame_info, sizeof(info), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(chain, cd.chain_header, sizeof(chain), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(matches.data(), xd.matches, cap * sizeof(lmx_match_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(leaders.data(), cd.leaders, cap_clusters * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(poses.data(), cd.poses, cap_clusters * sizeof(lmx_pose_refine_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(checks.data(), cd.checks, cap_clusters * sizeof(lmx_pose_verify_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(keep.data(), cd.keep, cap_clusters, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    // after the one synchronisation: the frame's filter record, as the chain's first launch left it
    std::vector<uint16_t> filtered(px);
    lmx_scene_filter_info fi;
    lmx::linemod::check(lmx_debug_scene_filtered(renders.handle(), 0, filtered.data(), &fi));
    size_t zeroed = 0;
    for (size_t i = 0; i < px; ++i) zeroed += depth[i] != 0 && filtered[i] == 0;
    std::printf("filter valid %lld sparse %lld scored %lld removed %lld sum_q %lld sum_qq %lld threshold %.17g zeroed %zu\n", (long long)fi.n_valid, (long long)fi.n_sparse,
                (long long)fi.n_scored, (long long)fi.n_removed, (long long)fi.sum_q, (long long)fi.sum_qq, fi.threshold, zeroed);
    std::printf("templates %zu matches %u clusters %u status %d\n", n_templates, header[2], header[3], info[6]);
    std::printf("chain live %u flags %u refined %u verified %u kept %u\n", chain[0], chain[1], chain[2], chain[3], chain[4]);
    for (uint32_t k = 0; k < chain[0]; ++k) {
      if (leaders[k] < 0) { std::printf("cluster %u dead\n", k); continue; }
      const lmx_match_t& m = matches[(size_t)leaders[k]];
      const lmx_pose_refine_t& p = poses[k];
      const lmx_pose_verify_t& v = checks[k];
      std::printf("cluster %u leader %d %d %d pose status %d iterations %d t %.17g %.17g %.17g verify status %d points %d %d %d scene %d cells %d roi %d %d %d %d rate %.17g %s\n", k,
                  m.x, m.y, m.template_id, p.status, p.iterations, p.t_mm[0], p.t_mm[1], p.t_mm[2], v.status, v.n_model, v.n_tested, v.n_occupied, v.n_scene, v.cells,
                  v.roi[0], v.roi[1], v.roi[2], v.roi[3], v.rate, keep[k] ? "kept" : "erased");
    }
    lmx::linemod::check(lmx_ctx_release(ctx));
    for (void* p : {(void*)xd.header, (void*)xd.frame_info, (void*)xd.matches, (void*)xd.diffs, (void*)xd.clusters_out, (void*)xd.members, (void*)cd.chain_header,
                    (void*)cd.leaders, (void*)cd.poses, (void*)cd.checks, (void*)cd.keep, (void*)d_bgr, (void*)d_depth})
      HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(stream));
    lmx_renderer_params_free(side);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
