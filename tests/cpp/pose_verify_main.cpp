// A complete caller of the pose verification through the C++ facade (include/lmx_linemod.hpp): trains a small bank from a mesh, keeps the
// templates' depth renders on the device, matches a scene, clusters with the depth values, refines the leader of every cluster against
// the scene depth, verifies the refined poses against the scene's voxel occupancy and prints which clusters are kept: the reference's
// detect callback from the match up to hypothesisVerification (src/linemod_carmine_detect.cpp:333-461, src/rgbdDetector.cpp:1457-1506).
// Prints what tests/test_gpu_pose_verify_cpp.py compares with the Python path.
//   pose_verify_main <triangles.f64> <views.f64> <width> <height> <focal> <scene_bgr.u8> <scene_depth.u16> <threshold> <collision_rate_threshold>
// triangles.f64: n x 9 doubles; views.f64: m x 10 doubles (R row major, distance); the scene files are dense rows.
#include <cstdio>
#include <cstdlib>
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
  if (argc != 10) {
    std::fprintf(stderr, "usage: pose_verify_main triangles.f64 views.f64 width height focal scene_bgr.u8 scene_depth.u16 threshold collision_rate_threshold\n");
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
    const double collision_rate_threshold = std::atof(argv[9]);
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

    const lmx::linemod::Image color{bgr.data(), cam.height, cam.width, 3, 1, (size_t)cam.width * 3};
    const lmx::linemod::Image depth_img{depth.data(), cam.height, cam.width, 1, 2, (size_t)cam.width * 2};
    std::vector<lmx::linemod::Match> found;
    det.match({color, depth_img}, (float)std::atof(argv[8]), found);
    std::vector<lmx_match_t> matches;
    for (const lmx::linemod::Match& m : found) matches.push_back(lmx_match_t{m.x, m.y, m.similarity, m.template_id, 0});
    const std::vector<lmx_depth_diff_t> diffs = renders.diff(depth_img, matches);
    std::vector<double> values;
    for (const lmx_depth_diff_t& d : diffs) values.push_back(lmx::linemod::DepthTemplates::value(d));

    lmx_cluster_params pp;
    pp.vote_row_col_step = 10; pp.renderer_radius_min = 0.4; pp.renderer_radius_step = 0.05; pp.cluster_size_thresh = 2;
    std::vector<lmx_cluster_t> clusters(matches.size() + 1);
    std::vector<int32_t> members(matches.size() + 1);
    size_t n_clusters = 0;
    lmx::linemod::check(lmx_cluster_matches_scored(matches.data(), matches.size(), values.data(), side->obj_origin_dists, side->rects, n_templates, &pp,
                                                   clusters.data(), clusters.size(), &n_clusters, members.data(), members.size()));
    std::printf("templates %zu matches %zu clusters %zu\n", n_templates, matches.size(), n_clusters);

    // each cluster's leader: its member of highest similarity, the first on a tie
    std::vector<lmx_match_t> leaders;
    for (size_t k = 0; k < n_clusters; ++k) {
      const lmx_cluster_t& c = clusters[k];
      int32_t best = members[c.member_begin];
      for (int32_t q = 1; q < c.member_count; ++q) {
        const int32_t i = members[c.member_begin + q];
        if (matches[i].similarity > matches[best].similarity) best = i;
      }
      leaders.push_back(matches[best]);
    }
    // the scene is uploaded once and stays in the object for both stages; the crops were rendered with the camera the scene was taken with
    renders.uploadScene({depth_img});
    lmx_pose_refine_params rp = lmx::linemod::DepthTemplates::poseRefineDefaults();
    rp.model_fx = rp.scene_fx = cam.fx; rp.model_fy = rp.scene_fy = cam.fy;
    rp.model_cx = rp.scene_cx = cam.cx; rp.model_cy = rp.scene_cy = cam.cy;
    const std::vector<lmx_pose_refine_t> poses = renders.refinePoses(leaders, rp);
    lmx_pose_verify_params vp = lmx::linemod::DepthTemplates::poseVerifyDefaults();
    vp.model_fx = vp.scene_fx = cam.fx; vp.model_fy = vp.scene_fy = cam.fy;
    vp.model_cx = vp.scene_cx = cam.cx; vp.model_cy = vp.scene_cy = cam.cy;
    const std::vector<lmx_pose_verify_t> checks = renders.verifyPoses(leaders, poses, vp);
    const std::vector<uint8_t> keep = lmx::linemod::DepthTemplates::keepVerified(checks, collision_rate_threshold);
    for (size_t k = 0; k < checks.size(); ++k) {
      const lmx_pose_verify_t& v = checks[k];
      std::printf("cluster %zu leader %d %d %d pose status %d verify status %d points %d %d %d scene %d cells %d roi %d %d %d %d rate %.17g %s\n", k, leaders[k].x,
                  leaders[k].y, leaders[k].template_id, poses[k].status, v.status, v.n_model, v.n_tested, v.n_occupied, v.n_scene, v.cells, v.roi[0], v.roi[1], v.roi[2],
                  v.roi[3], v.rate, keep[k] ? "kept" : "erased");
    }
    lmx_renderer_params_free(side);
  } catch (const lmx::linemod::Exception& e) {
    std::fprintf(stderr, "exception status %d: %s\n", (int)e.status, e.what());
    return 1;
  }
  return 0;
}
