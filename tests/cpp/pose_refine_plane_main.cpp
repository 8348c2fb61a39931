// A complete caller of the point-to-plane pose refinement through the C++ facade (include/lmx_linemod.hpp): keeps one depth crop on the
// device, enables the normals, sets a refinement schedule and the stages' point_shift (DepthTemplates::setRefinePlane), reads the shifts
// back, refines a list of matches against a scene depth frame under them, then clears the shifts and refines the same matches again.
// Prints what tests/test_gpu_pose_refine_plane.py compares with the Python path.
//   pose_refine_plane_main <crop.u16> <w> <h> <rect_x> <rect_y> <scene.u16> <W> <H> <fx> <fy> <cx> <cy> <schedule> <shifts> <x,y> [<x,y> ...]
// schedule: "stride:iterations:max_dist:radius,..." with the defaults' eps, or "-" for none; shifts: "8,-1,..."; the files are dense rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "lmx_linemod.hpp"

static std::vector<uint16_t> read_u16(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(1); }
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<uint16_t> out(raw.size() / 2);
  std::memcpy(out.data(), raw.data(), out.size() * 2);
  return out;
}

static void print_records(const char* what, const std::vector<lmx_match_t>& matches, const std::vector<lmx_pose_refine_t>& poses) {
  for (size_t k = 0; k < poses.size(); ++k) {
    const lmx_pose_refine_t& p = poses[k];
    std::printf("%s match %d %d status %d stage %d iterations %d pairs %d %d rms %.17g %.17g R", what, matches[k].x, matches[k].y, p.status, p.reserved, p.iterations,
                p.n_pairs_first, p.n_pairs_last, p.rms_first_mm, p.rms_last_mm);
    for (double v : p.R) std::printf(" %.17g", v);
    std::printf(" t %.17g %.17g %.17g\n", p.t_mm[0], p.t_mm[1], p.t_mm[2]);
  }
}

int main(int argc, char** argv) {
  if (argc < 16) { std::fprintf(stderr, "usage: pose_refine_plane_main crop.u16 w h rect_x rect_y scene.u16 W H fx fy cx cy schedule shifts x,y [x,y ...]\n"); return 2; }
  try {
    const std::vector<uint16_t> crop = read_u16(argv[1]), scene = read_u16(argv[6]);
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), W = std::atoi(argv[7]), H = std::atoi(argv[8]);
    if (crop.size() != (size_t)w * h || scene.size() != (size_t)W * H) { std::fprintf(stderr, "the files do not hold %d x %d and %d x %d pixels\n", w, h, W, H); return 2; }
    const int32_t rects[4] = {std::atoi(argv[4]), std::atoi(argv[5]), w, h};

    lmx_pose_refine_params rp = lmx::linemod::DepthTemplates::poseRefineDefaults();
    rp.model_fx = rp.scene_fx = std::atof(argv[9]); rp.model_fy = rp.scene_fy = std::atof(argv[10]);
    rp.model_cx = rp.scene_cx = std::atof(argv[11]); rp.model_cy = rp.scene_cy = std::atof(argv[12]);
    rp.max_iterations = 5;   // the metric is meant for few iterations
    rp.rects = rects;

    std::vector<lmx_pose_refine_stage> stages;
    for (const char* s = std::strcmp(argv[13], "-") ? argv[13] : ""; *s;) {
      lmx_pose_refine_stage st = lmx_pose_refine_stage();
      if (std::sscanf(s, "%d:%d:%lf:%d", &st.stride, &st.max_iterations, &st.max_dist_mm, &st.search_radius) != 4) { std::fprintf(stderr, "bad schedule at '%s'\n", s); return 2; }
      st.eps_rot_rad = rp.eps_rot_rad; st.eps_trans_mm = rp.eps_trans_mm;
      stages.push_back(st);
      const char* comma = std::strchr(s, ',');
      s = comma ? comma + 1 : s + std::strlen(s);
    }
    std::vector<int32_t> shifts;
    for (const char* s = argv[14]; *s;) {
      shifts.push_back(std::atoi(s));
      const char* comma = std::strchr(s, ',');
      s = comma ? comma + 1 : s + std::strlen(s);
    }
    std::vector<lmx_match_t> matches;
    for (int k = 15; k < argc; ++k) {
      int x = 0, y = 0;
      if (std::sscanf(argv[k], "%d,%d", &x, &y) != 2) { std::fprintf(stderr, "bad match '%s'\n", argv[k]); return 2; }
      matches.push_back(lmx_match_t{x, y, 90.0f, 0, 0});
    }

    lmx::linemod::DepthTemplates renders;
    renders.fromCrops({crop.data()}, {{w, h}});
    const lmx::linemod::Image depth{scene.data(), H, W, 1, 2, (size_t)W * 2};

    renders.enableNormals(rp.scene_fx, rp.scene_fy);   // the scene's normals are computed with these, once per staged scene
    renders.setRefineSchedule(stages);
    renders.setRefinePlane(shifts);
    std::printf("plane");
    for (int32_t k : renders.refinePlane()) std::printf(" %d", k);
    std::printf("\n");
    print_records("plane", matches, renders.refinePoses(matches, rp, depth));

    renders.setRefinePlane({});
    std::printf("plane cleared %zu\n", renders.refinePlane().size());
    print_records("point", matches, renders.refinePoses(matches, rp, depth));
  } catch (const lmx::linemod::Exception& e) {
    std::fprintf(stderr, "exception status %d: %s\n", (int)e.status, e.what());
    return 1;
  }
  return 0;
}
