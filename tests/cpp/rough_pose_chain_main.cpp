// A complete C++ caller of the rough pose chain (include/lmx.h: lmx_rough_pose_chain_on, through DepthTemplates::roughPoseChain of
// include/lmx_linemod.hpp): trains a small bank from a mesh, uploads the frame to the device, enqueues, uploads the scene, exports the
// depth-scored clusters and runs the rough pose of every cluster, its refinement and its verification on one stream, with nothing read on
// the host in between: the reference's detect callback from the match through getRoughPoseByClustering up to hypothesisVerification.
// Device memory is read back only to print what tests/test_gpu_rough_pose_cpp.py compares with the Python path.
//   rough_pose_chain_main <triangles.f64> <views.f64> <width> <height> <focal> <scene_bgr.u8> <scene_depth.u16> <threshold>
//                         <collision_rate_threshold> <orientation_threshold_deg> <window>
#include <hip/hip_runtime_api.h>

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
  if (argc != 12) {
    std::fprintf(stderr, "usage: rough_pose_chain_main triangles.f64 views.f64 width height focal scene_bgr.u8 scene_depth.u16 threshold collision_rate_threshold "
                         "orientation_threshold_deg window\n");
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

    const size_t cap = 1 << 14, cap_clusters = 256;
    const int window = std::atoi(argv[11]);
    lmx_rough_model* model = nullptr;
    lmx::linemod::check(lmx_rough_model_create(0, tri.data(), (int32_t)(tri.size() / 9), &cam, template_views.data(), (int32_t)n_templates, nullptr, side->obj_origin_dists,
                                               (int32_t)cap_clusters, window, window, &model));

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
    renders.uploadSceneDevice({depth_img}, stream);

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

    lmx_pose_refine_params rp = lmx::linemod::DepthTemplates::poseRefineDefaults();
    rp.model_fx = rp.scene_fx = cam.fx; rp.model_fy = rp.scene_fy = cam.fy;
    rp.model_cx = rp.scene_cx = cam.cx; rp.model_cy = rp.scene_cy = cam.cy;
    lmx_pose_verify_params vp = lmx::linemod::DepthTemplates::poseVerifyDefaults();
    vp.model_fx = vp.scene_fx = cam.fx; vp.model_fy = vp.scene_fy = cam.fy;
    vp.model_cx = vp.scene_cx = cam.cx; vp.model_cy = vp.scene_cy = cam.cy;
    lmx_rough_chain_desc cd;
    std::memset(&cd, 0, sizeof(cd));
    cd.class_index = -1;
    cd.refine = &rp; cd.verify = &vp;
    cd.keep_thresh = std::atof(argv[9]);
    lmx::linemod::check(lmx_rough_trace_min(std::atof(argv[10]), &cd.trace_min));
    cd.header = xd.header; cd.frame_info = xd.frame_info;
    cd.matches = xd.matches; cd.cap_matches = cap;
    cd.clusters = xd.clusters_out; cd.cap_clusters = cap_clusters;
    cd.members = xd.members; cd.cap_members = cap;
    cd.chain_header = device_array<uint32_t>(8);
    cd.rough = device_array<lmx_rough_pose_t>(cap_clusters);
    cd.member_group = device_array<int32_t>(cap);
    cd.poses = device_array<lmx_pose_refine_t>(cap_clusters);
    cd.checks = device_array<lmx_pose_verify_t>(cap_clusters);
    cd.keep = device_array<uint8_t>(cap_clusters);
    renders.roughPoseChain(model, cd, stream);

    // only to print: the copies back on the same stream, and the one synchronisation of this program
    uint32_t header[16], chain[8];
    int32_t info[8];
    std::vector<lmx_rough_pose_t> rough(cap_clusters);
    std::vector<lmx_pose_refine_t> poses(cap_clusters);
    std::vector<lmx_pose_verify_t> checks(cap_clusters);
    std::vector<uint8_t> keep(cap_clusters);
    HIP_OK(hipMemcpyAsync(header, xd.header, sizeof(header), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(info, xd.frame_info, sizeof(info), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(chain, cd.chain_header, sizeof(chain), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(rough.data(), cd.rough, cap_clusters * sizeof(lmx_rough_pose_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(poses.data(), cd.poses, cap_clusters * sizeof(lmx_pose_refine_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(checks.data(), cd.checks, cap_clusters * sizeof(lmx_pose_verify_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(keep.data(), cd.keep, cap_clusters, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    std::printf("templates %zu matches %u clusters %u status %d\n", n_templates, header[2], header[3], info[6]);
    std::printf("chain live %u flags %u refined %u verified %u kept %u rough %u\n", chain[0], chain[1], chain[2], chain[3], chain[4], chain[5]);
    for (uint32_t k = 0; k < chain[0]; ++k) {
      const lmx_rough_pose_t& r = rough[k];
      const lmx_pose_refine_t& p = poses[k];
      const lmx_pose_verify_t& v = checks[k];
      std::printf("cluster %u rough status %d members %d groups %d group %d of %d front %d at %d %d distance %.17g R0 %.17g rect %d %d %d %d points %d "
                  "pose status %d iterations %d t %.17g %.17g %.17g verify status %d points %d %d %d rate %.17g %s\n",
                  k, r.status, r.n_members, r.n_groups, r.group, r.n_group_members, r.front, r.x, r.y, r.distance, r.R[0], r.rect[0], r.rect[1], r.rect[2], r.rect[3],
                  r.n_model, p.status, p.iterations, p.t_mm[0], p.t_mm[1], p.t_mm[2], v.status, v.n_model, v.n_tested, v.n_occupied, v.rate, keep[k] ? "kept" : "erased");
    }
    lmx::linemod::check(lmx_ctx_release(ctx));
    for (void* p : {(void*)xd.header, (void*)xd.frame_info, (void*)xd.matches, (void*)xd.diffs, (void*)xd.clusters_out, (void*)xd.members, (void*)cd.chain_header,
                    (void*)cd.rough, (void*)cd.member_group, (void*)cd.poses, (void*)cd.checks, (void*)cd.keep, (void*)d_bgr, (void*)d_depth})
      HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(stream));
    lmx_rough_model_free(model);
    lmx_renderer_params_free(side);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
