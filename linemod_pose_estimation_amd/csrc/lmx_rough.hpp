// What lmx_rough.hip (the model object, the group and render kernels) and lmx_verify.hip (lmx_rough_pose_chain_on, which runs the refine and
// verify bodies behind them) share.  The arithmetic is lmx_rough_pose.hpp and lmx_mesh_raster.hpp.
#pragma once

#include <mutex>

#include "lmx_internal.hpp"
#include "lmx_mesh_raster.hpp"
#include "lmx_rough_pose.hpp"

namespace lmx {
namespace rp {

struct CropEntry { const uint16_t* data; int32_t w, h, pitch, pad; };   // the bytes of lmx_verify.hip's DepthCrop
// What the two pose kernels run for a slot.  run 0: zeroed records.  The crop is the slot's window: x, y place its corner in the scene,
// rect_x, rect_y in the model camera; lat_x, lat_y: the corner of the render's silhouette box inside the window, where the pixel lattice of
// a refinement stage of stride > 1 starts (lmx_pose_refine.hpp, SCHEDULE: the crop of a rough pose is that box).
struct Job { int32_t run, frame, x, y, rect_x, rect_y, lat_x, lat_y; };
static_assert(sizeof(CropEntry) == 24 && sizeof(Job) == 32, "layouts the kernels rely on");

struct StageArgs {
  pc::Lists L;               // what an export wrote, device memory
  int32_t class_index;
  double trace_min;
  uint32_t* chain_header;    // [pc::C_WORDS], zeroed in front of the first kernel
  Record* rough;             // [cap_clusters]
  int32_t* member_group;     // [cap_members]
};

}  // namespace rp
}  // namespace lmx

struct lmx_rough_model {
  int32_t device = 0;
  std::mutex m;
  lmx::mr::Camera cam = {};
  int32_t n_tri = 0, n_views = 0, cap_slots = 0, win_w = 0, win_h = 0;
  size_t win_stride = 0;                 // elements of a slot's window: win_h rows of crop_pitch(win_w)
  double* d_tri = nullptr;               // [n_tri][9]
  lmx::rp::View* d_views = nullptr;      // [n_views]
  double* d_slot_view = nullptr;         // [cap_slots][10]: R, distance of the slot's mean view
  int32_t* d_state = nullptr;            // [cap_slots][kMeshStateWords]
  lmx::mr::Tri* d_work = nullptr;        // [cap_slots][n_tri]
  uint16_t* d_window = nullptr;          // [cap_slots][win_stride]
  lmx::rp::CropEntry* d_crops = nullptr; // [cap_slots]
  lmx::rp::Job* d_jobs = nullptr;        // [cap_slots]
  size_t bytes = 0;
  // the kernels of a call run on the calling lmx_depth_templates' stream; `done` is recorded behind them, and the next call's stream waits for it
  hipEvent_t done = nullptr;
  bool done_pending = false;
};

namespace lmx {
// k_rough_group, k_rough_setup, k_rough_raster, k_rough_finish on `s` for the slots 0 .. a.L.cap_clusters - 1 (<= m->cap_slots): behind them
// rough, member_group, chain_header[0], [1], [5], m->d_crops and m->d_jobs are final.
void launch_rough_stage(hipStream_t s, const lmx_rough_model* m, const rp::StageArgs& a);
}  // namespace lmx
