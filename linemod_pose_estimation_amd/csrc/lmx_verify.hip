// Depth check of matches against the rendered depth of their templates (include/lmx.h: lmx_depth_templates_*, lmx_depth_diff_matches): the
// depth half of the reference's depth_normal_diff_calc (src/rgbdDetector.cpp:147-282) with the renders made once instead of per match.
// The arithmetic is lmx_depth_verify.hpp; this file is the storage and the parallel shape:
//
//   atlas          every template's depth render cropped to its silhouette box, rows padded with zeros to 16 bytes, every crop 16-byte
//                  aligned, in chunks of device memory (from_mesh: one per render batch, sized to that batch's crops; from_crops: one);
//                  a table entry per template {address, w, h, pitch}
//   k_depth_crop   from_mesh: copies each view's silhouette box out of the batch's depth planes into its chunk, writing the padding
//   k_walk<NORMALS, SRC>   the crop walk (diff_walk), one 256-lane workgroup per item.  Lanes run along crop rows, one aligned 16-byte vector
//                  (8 pixels) each; a crop narrower than 64 vectors packs several rows into a wave; waves take rows (groups of rows) in
//                  turn.  Scene pixels are read as uint16 under the in-image predicate of lmx_depth_verify.hpp and nowhere else.  Per-lane
//                  sums are 64-bit; wave shuffles, then LDS across the four waves, then one 16-byte store.  No atomics, no workgroup waits
//                  for another.  SRC says what an item is (walk_item): a job of the host's match list against the frames its call staged,
//                  or a RAW record of an output slot -- un-classed or classed -- against the scene lmx_depth_templates_upload_scene left on
//                  the device: the input of the scored consumer chain (lmx_f2.hip).  All take one argument struct (WalkArgs)
//   scene          one pinned staging buffer and one device buffer per object.  lmx_depth_diff_matches stages the frames that have matches
//                  and waits for its results; upload_scene stages all frames, records an event behind their copies and returns
// The normal term (lmx_depth_templates_enable_normals, lmx_normal_diff_matches; arithmetic: lmx_normal_verify.hpp), only for an object that
// enabled it:
//   k_normal_map_crops / k_normal_map_frames   depth -> packed normals, one pixel per lane, the nine depth reads straight from L2 under the
//                  in-image predicate, one 8-byte store per pixel.  Crops: once per enable_normals, all crops in one launch, into chunks that
//                  mirror the depth chunks (same pitch: the padding's normals are zeros).  Scene frames: once per scene, when a normal-scored
//                  call first needs them, on that call's stream behind the scene's event
//   k_walk<true, SRC>   the NORMALS instantiations of the same walk, both terms in one pass (nv::add_vector): the two stored normals of a
//                  pixel are read next to its two depths, their angle comes out of the chord table in global memory
//   k_walk_records_dev<NORMALS, CLASSES>   the record sources for a caller that has not read the slot's header (lmx_ctx_export_clusters_on):
//                  persistent workgroups that take the record count from device memory; see the kernel
// Pose refinement (lmx_pose_refine_matches; arithmetic and control: lmx_pose_refine.hpp), on the same table and scene:
//   k_pose_refine  one 256-lane workgroup per match, the same walk over the crop's vectors once per pass, every pass of a job inside one
//                  launch; under a refinement schedule (lmx_depth_templates_set_refine_schedule) every pass of every stage, a stage of
//                  stride > 1 walking a pixel lattice spread over the lanes instead; see the kernel.  Its PLANE instantiation (and those
//                  of the two cluster kernels below) runs only when a stage in force has a point_shift >= 0
//                  (lmx_depth_templates_set_refine_plane): such a stage adds the 29 point-to-plane sums against the scene's normals
// Pose verification (lmx_pose_verify_matches; arithmetic: lmx_pose_verify.hpp), the stage after it:
//   k_pose_verify  one 256-lane workgroup per match: the crop walk for the voxel grid's extent, a 32 KiB occupancy bitmap in LDS marked
//                  from the scene pixels of the posed model's region, the crop walk again to count the points in marked voxels; see the kernel
// Both stages on the clusters an export left in device memory (lmx_pose_chain_on; the decisions on the lists: lmx_pose_chain.hpp):
//   k_pose_refine_clusters / k_pose_verify_clusters   one workgroup per cluster slot, the leader and its job found on the device, then the
//                  bodies of the two kernels above; see the kernels
// The same two bodies behind the rough pose stage (lmx_rough_pose_chain_on; the stage itself: lmx_rough.hip, lmx_rough_pose.hpp):
//   k_rough_refine_clusters / k_rough_verify_clusters   one workgroup per cluster slot on the job and the rendered crop the stage left
// The scene filter (lmx_depth_templates_set_scene_filter; arithmetic: lmx_scene_filter.hpp, kernels: lmx_scene_filter.hip), only for an object
// that set it: a filtered copy of the scene next to d_scene, made once per scene on the object's stream when a pose stage first needs it
// (pose_scene_on); the five pose launch sites pass it where they pass d_scene otherwise.
// The host half has one launch site for every walk kernel (depth_launch_walk), one body for both match-list paths
// (diff_selected), one guard in front of every normal-scored call (need_normals) and one body around the launch of both pose stages
// (pose_call).
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "lmx_internal.hpp"
#include "lmx_depth_verify.hpp"
#include "lmx_normal_verify.hpp"
#include "lmx_pose_refine.hpp"
#include "lmx_pose_verify.hpp"
#include "lmx_pose_chain.hpp"
#include "lmx_mesh_raster.hpp"
#include "lmx_export_pack.hpp"
#include "lmx_rough.hpp"
#include "lmx_scene_filter.hpp"

namespace lmx {
struct DepthJob { int32_t x, y, template_id, frame; };   // frame: index among the frames uploaded for this call
namespace {

struct DepthCrop {          // table entry: 24 bytes per template
  const uint16_t* data;     // [h][pitch], 16-byte aligned; null for an empty crop
  int32_t w, h, pitch, pad;
};
static_assert(sizeof(DepthCrop) == 24 && sizeof(DepthJob) == 16 && sizeof(lmx_depth_diff_t) == 16, "layouts the kernels rely on");
static_assert(sizeof(lmx_normal_diff_t) == 16 && sizeof(nv::Packed) == 8, "layouts the kernels rely on");
static_assert(dv::kWalkLanes == 64, "the lanes along a crop row are those of one wave (lane = tid & 63, wave_sum)");

constexpr int kCropBatch = 32;   // views rendered per batch (as lmx_mesh_render)
struct CropBatch { uint64_t dst_elem[kCropBatch]; };   // where view v's crop starts in the batch's chunk, in elements

__global__ __launch_bounds__(256) void k_depth_crop(const uint16_t* __restrict__ depth, const int32_t* __restrict__ state, int W, int H,
                                                    uint16_t* __restrict__ chunk, CropBatch where) {
  const int v = blockIdx.y;
  const int32_t* b = state + (size_t)v * kMeshStateWords + MS_LEVEL;   // {xmin, ymin, xmax, ymax} of the covered pixels, inside the image
  if (b[2] < 0) return;
  const int x0 = b[0], y0 = b[1], w = b[2] - b[0] + 1, h = b[3] - b[1] + 1;
  const int vpr = dv::crop_pitch(w) / dv::kPitchAlign;
  const uint16_t* src = depth + (size_t)v * H * W;
  uint16_t* dst = chunk + where.dst_elem[v];
  for (int q = blockIdx.x * 256 + threadIdx.x; q < h * vpr; q += gridDim.x * 256) {
    const int row = q / vpr, c0 = (q - row * vpr) * dv::kPitchAlign;
    const uint16_t* s = src + (size_t)(y0 + row) * W + x0;
    uint32_t word[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = c0 + 2 * k < w ? s[c0 + 2 * k] : 0u, hi = c0 + 2 * k + 1 < w ? s[c0 + 2 * k + 1] : 0u;   // the padding is zeros
      word[k] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4*>(dst + (size_t)q * dv::kPitchAlign) = make_uint4(word[0], word[1], word[2], word[3]);
  }
}

// One aligned 16-byte load.  The crop's address comes out of the table, so the compiler cannot know that it is global memory and would
// emit a flat load; told here, it emits a global one.
__device__ __forceinline__ uint4 load_global_16(const uint16_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = *(const __attribute__((address_space(1))) u32x4*)p;
  return make_uint4(v.x, v.y, v.z, v.w);
#else
  return *reinterpret_cast<const uint4*>(p);
#endif
}

// ---- the normal maps (only for an object that enabled normals) -----------------------------------------------------------------------------------------
// Normals of one w x h depth image with rows of `pitch` elements into dst[h][pitch], by the workgroups blockIdx.x, blockIdx.x + gridDim.x, ...
// of 256 pixels each; elements past w (a crop's padding) get zeros.  Every depth read lies inside [0, w) x [0, h) (nv::depth_or_zero).
__device__ __forceinline__ void normal_map_image(const uint16_t* __restrict__ src, int w, int h, int pitch, nv::Packed* __restrict__ dst, const nv::Params p) {
  const int n = h * pitch;   // <= 2^28 (dv::kMaxCropSide) for a crop, W * H of a camera frame for the scene
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
    const int y = q / pitch, x = q - y * pitch;
    dst[q] = x < w ? nv::normal_at(src, w, h, (size_t)pitch, x, y, p) : (nv::Packed)0;
  }
}

__global__ __launch_bounds__(256) void k_normal_map_crops(const DepthCrop* __restrict__ crops, nv::Packed* const* __restrict__ normals, nv::Params p) {
  const DepthCrop c = crops[blockIdx.y];
  if (c.w <= 0 || c.h <= 0) return;
  normal_map_image(c.data, c.w, c.h, c.pitch, normals[blockIdx.y], p);
}

__global__ __launch_bounds__(256) void k_normal_map_frames(const uint16_t* __restrict__ scene, int W, int H, nv::Packed* __restrict__ out, nv::Params p) {
  const size_t frame = (size_t)blockIdx.y * H * W;
  normal_map_image(scene + frame, W, H, W, out + frame, p);
}

// ---- the crop walk ------------------------------------------------------------------------------------------------------------------------------------
// The zeroed record of what is no job: the record's 8-byte words over the first lanes of the workgroup.
template <typename T>
__device__ __forceinline__ void store_zero_record(T* p, int tid) {
  if (tid < (int)(sizeof(T) / 8)) reinterpret_cast<long long*>(p)[tid] = 0;
}

// The 16-byte result of a match, and with NORMALS the 16 bytes of its normal term.
template <bool NORMALS>
__device__ __forceinline__ void store_sums(lmx_depth_diff_t* __restrict__ out, lmx_normal_diff_t* __restrict__ nout, unsigned long long sum, int n_valid,
                                           int n_template, unsigned long long angle, int n_normal) {
  *reinterpret_cast<int4*>(out) = make_int4((int)(uint32_t)sum, (int)(uint32_t)(sum >> 32), n_valid, n_template);
  if constexpr (NORMALS) *reinterpret_cast<int4*>(nout) = make_int4((int)(uint32_t)angle, (int)(uint32_t)(angle >> 32), n_normal, 0);
}

// The crop walk of one match of template `id` at (x, y) against scene frame `f`, by a whole 256-lane workgroup: every walk kernel below ends
// in it.  Lanes run along crop rows, one aligned vector each (dv::add_vector).  With NORMALS both terms in the same pass (nv::add_vector):
// a lane reads its eight crop normals as four aligned 16-byte vectors next to the crop's depths, the scene's normals next to the scene's
// depths, the angles out of the chord table; without, normals / scene_normals / table / nout are not looked at.  What is no job (is_job
// false, or an empty crop) gets zeros without a look at the table or the scene: the same for every lane, before any barrier.  Every lane of
// the workgroup must arrive (it holds a barrier); lane 0 stores the result.
template <bool NORMALS>
__device__ __forceinline__ void diff_walk(const DepthCrop* __restrict__ crops, nv::Packed* const* __restrict__ normals, bool is_job, int32_t id, int32_t x, int32_t y,
                                          int32_t f, const uint16_t* __restrict__ scene, const nv::Packed* __restrict__ scene_normals, int W, int H,
                                          const uint32_t* __restrict__ table, lmx_depth_diff_t* __restrict__ out, lmx_normal_diff_t* __restrict__ nout) {
  __shared__ unsigned long long s_sum[NORMALS ? 8 : 4];   // per wave: sum_abs_mm, then sum_angle_urad
  __shared__ int s_count[NORMALS ? 12 : 8];               // per wave: n_valid, n_template, then n_normal
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const DepthCrop c = is_job ? crops[id] : DepthCrop{nullptr, 0, 0, 0, 0};
  if (c.w <= 0 || c.h <= 0) {
    if (tid == 0) store_sums<NORMALS>(out, nout, 0, 0, 0, 0, 0);
    return;
  }
  const uint16_t* frame = scene + (size_t)f * H * W;
  const int vpr = c.pitch / dv::kPitchAlign;        // vectors in a row
  const int lanes_per_row = vpr < dv::kWalkLanes ? vpr : dv::kWalkLanes;
  const int rows_per_pass = dv::kWalkLanes / lanes_per_row;     // rows a wave takes at once
  const int sub = lane / lanes_per_row, v0 = lane - sub * lanes_per_row;
  dv::Sums a = {0, 0, 0};
  nv::Sums b = {0, 0};
  for (int row0 = wave * rows_per_pass; row0 < c.h; row0 += 4 * rows_per_pass) {
    const int i = row0 + sub;
    if (sub >= rows_per_pass || i >= c.h) continue;
    int32_t Y = 0;
    const bool row_in = dv::scene_row(y, i, H, &Y);
    const uint16_t* trow = c.data + (size_t)i * c.pitch;
    const uint16_t* srow = frame + (size_t)Y * W;     // Y = 0 when the row lies outside: never read then
    for (int v = v0; v < vpr; v += lanes_per_row) {
      const int col0 = v * dv::kPitchAlign;
      const uint4 q = load_global_16(trow + col0);    // past w: the padding, zeros
      const uint32_t word[4] = {q.x, q.y, q.z, q.w};
      if constexpr (NORMALS) {
        const nv::Packed* nvec = normals[id] + (size_t)i * c.pitch + col0;   // 64 contiguous, 16-byte aligned bytes
        nv::Packed tn[dv::kPitchAlign];
#pragma unroll
        for (int k = 0; k < dv::kPitchAlign / 2; ++k) {
          const uint4 n2 = load_global_16(reinterpret_cast<const uint16_t*>(nvec + 2 * k));
          tn[2 * k] = (nv::Packed)n2.x | ((nv::Packed)n2.y << 32);
          tn[2 * k + 1] = (nv::Packed)n2.z | ((nv::Packed)n2.w << 32);
        }
        nv::add_vector(word, tn, row_in, x, col0, W, srow, scene_normals + (srow - scene), table, &a, &b);   // the same row of the scene's normals
      } else {
        dv::add_vector(word, row_in, x, col0, W, srow, &a);
      }
    }
  }
  const unsigned long long sum = wave_sum<unsigned long long>(a.sum_abs_mm);
  const int n_valid = wave_sum(a.n_valid), n_template = wave_sum(a.n_template);
  if (lane == 0) { s_sum[wave] = sum; s_count[wave] = n_valid; s_count[4 + wave] = n_template; }
  if constexpr (NORMALS) {
    const unsigned long long angle = wave_sum<unsigned long long>(b.sum_angle_urad);
    const int n_normal = wave_sum(b.n_normal);
    if (lane == 0) { s_sum[4 + wave] = angle; s_count[8 + wave] = n_normal; }
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long total[2] = {0, 0};
    int count[3] = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      total[0] += s_sum[w]; count[0] += s_count[w]; count[1] += s_count[4 + w];
      if constexpr (NORMALS) { total[1] += s_sum[4 + w]; count[2] += s_count[8 + w]; }
    }
    store_sums<NORMALS>(out, nout, total[0], count[0], count[1], total[1], count[2]);
  }
}

// A RAW record of an output slot is a job unless the table does not hold its template, the scene does not hold its frame, or it is of another
// class (the device consumer chain carries the result, zeros then, through its sorts: lmx_f2.hip, SCORED and NORMAL).
__device__ __forceinline__ bool record_is_job(const lmx_raw_match_t& r, int32_t count, int32_t n_frames, int32_t class_index) {
  return r.template_id >= 0 && r.template_id < count && r.frame >= 0 && r.frame < n_frames && (class_index < 0 || r.class_index == class_index);
}

// The same for an object that holds several classes' crops one class after the other (lmx_depth_templates_append): class c's template i is
// crop class_base[c] + i.  No job, hence zeros and no walk, for a class >= n_classes, a template_id outside its class's range (it would be
// the next class's crop), a frame outside the scene.
__device__ __forceinline__ bool record_class_job(const lmx_raw_match_t& r, const int32_t* __restrict__ class_base, int32_t n_classes, int32_t n_frames, int32_t* id) {
  *id = 0;
  if (r.class_index < 0 || r.class_index >= n_classes || r.frame < 0 || r.frame >= n_frames) return false;
  const int32_t first = class_base[r.class_index], end = class_base[r.class_index + 1];
  if (r.template_id < 0 || r.template_id >= end - first) return false;
  *id = first + r.template_id;
  return true;
}

// What every walk kernel takes, by value.  The items come from one of three sources: job i of the host's match list (its frame is its slot
// among the frames in `scene`), or RAW record i of an output slot against the scene upload_scene left on the device, under one of the two
// predicates above.
enum WalkSource { WALK_JOBS, WALK_RECORDS, WALK_RECORDS_CLASSES };
struct WalkArgs {
  const DepthCrop* crops;
  nv::Packed* const* normals;
  const uint32_t* hdr;              // k_walk_records_dev: the slot's header, [0] candidates, [1] records
  const lmx_raw_match_t* recs;      // the two record sources
  uint32_t cap;                     // k_walk_records_dev: of the slot's lists
  int32_t count;                    // WALK_RECORDS: templates in the table
  int32_t class_index;              // WALK_RECORDS: -1 = every class
  const int32_t* class_base;        // WALK_RECORDS_CLASSES: n_classes + 1 entries
  int32_t n_classes;
  const uint16_t* scene;
  const nv::Packed* scene_normals;
  int32_t n_frames, W, H;
  const uint32_t* table;
  lmx_depth_diff_t* diffs;
  lmx_normal_diff_t* ndiffs;
  const DepthJob* jobs;             // WALK_JOBS; last, so the record kernels keep the argument offsets they had
};
struct WalkItem { bool is_job; int32_t id, x, y, frame; };

// Item i of a source: walk_item; its record half, on a record the caller has loaded: record_item (k_walk_records_dev says why it loads itself).
template <int SRC>
__device__ __forceinline__ WalkItem record_item(const WalkArgs& a, const lmx_raw_match_t& r) {
  WalkItem it{false, r.template_id, r.x, r.y, r.frame};
  if constexpr (SRC == WALK_RECORDS_CLASSES) it.is_job = record_class_job(r, a.class_base, a.n_classes, a.n_frames, &it.id);
  else it.is_job = record_is_job(r, a.count, a.n_frames, a.class_index);
  return it;
}
template <int SRC>
__device__ __forceinline__ WalkItem walk_item(const WalkArgs& a, uint32_t i) {
  if constexpr (SRC == WALK_JOBS) {
    const DepthJob j = a.jobs[i];
    return WalkItem{true, j.template_id, j.x, j.y, j.frame};
  } else {
    const lmx_raw_match_t r = a.recs[i];
    return record_item<SRC>(a, r);
  }
}

// One workgroup per item: the depth term alone or both terms, times the three sources.  What is no job takes diff_walk's zero-store exit.
template <bool NORMALS, int SRC>
__global__ __launch_bounds__(256) void k_walk(const WalkArgs a) {
  const WalkItem it = walk_item<SRC>(a, blockIdx.x);
  diff_walk<NORMALS>(a.crops, a.normals, it.is_job, it.id, it.x, it.y, it.frame, a.scene, a.scene_normals, a.W, a.H, a.table, &a.diffs[blockIdx.x],
                     NORMALS ? &a.ndiffs[blockIdx.x] : nullptr);
}

// The record kernels again for a caller that does not know the record count (lmx_ctx_export_clusters_on: no host reads the slot):
// a fixed grid of persistent workgroups, workgroup b walks records b, b + gridDim.x, ... below hdr[1], which every lane reads from the
// slot's header in device memory; a list that overflowed is not walked at all (the pack kernel reports it).  Record i is a job or not by
// the same two predicates, and gets the same 16 (32) bytes from the same diff_walk.
// The one thing a second job of a workgroup adds: diff_walk's per-wave partial sums live in static LDS, and lane 0 still adds up the
// first job's while the other waves go on.  So ONE barrier stands in front of a walk that follows an earlier walk of the same workgroup
// (`dirty`), and none anywhere else: behind it lane 0 has left diff_walk, hence has read s_sum / s_count.  Records that are no job, and
// jobs with an empty crop, touch no LDS and take no barrier, however many lie between two walks; a workgroup's first walk takes none
// either.  Chosen over two alternating LDS sets: it leaves diff_walk as it is, and the wait is short -- the other waves spend it on
// the next record's load, which is issued in front of the barrier.  n, i and `walks` depend on the header, blockIdx and record i alone:
// every lane of a workgroup takes the same trips and the same branch around the barrier.
template <bool NORMALS, bool CLASSES>
__global__ __launch_bounds__(256) void k_walk_records_dev(const WalkArgs a) {
  const uint32_t n_cand = a.hdr[0], n = a.hdr[1];
  if (xpack::list_overflowed(n_cand, n, a.cap)) return;
  bool dirty = false;   // an earlier walk of this workgroup used the LDS sums
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    // loaded here, not inside walk_item: there the compiler splits the record's 12-byte load of {template_id, class_index, frame} in three and
    // puts the class's behind the template test -- a second memory round trip per record (profiles/walk_variants_refactor.txt)
    const lmx_raw_match_t r = a.recs[i];
    const WalkItem it = record_item<CLASSES ? WALK_RECORDS_CLASSES : WALK_RECORDS>(a, r);
    bool walks = false;
    if (it.is_job) { const DepthCrop c = a.crops[it.id]; walks = c.w > 0 && c.h > 0; }
    if (walks && dirty) __syncthreads();
    diff_walk<NORMALS>(a.crops, a.normals, it.is_job, it.id, it.x, it.y, it.frame, a.scene, a.scene_normals, a.W, a.H, a.table, &a.diffs[i],
                       NORMALS ? &a.ndiffs[i] : nullptr);
    dirty = dirty || walks;
  }
}

// ---- pose refinement (lmx_pose_refine_matches; arithmetic and control: lmx_pose_refine.hpp) ---------------------------------------------------------
struct PoseJob { int32_t x, y, template_id, frame, rect_x, rect_y, lat_x, lat_y; };   // frame: as DepthJob's; lat_x, lat_y: lattice_pixels' origin
static_assert(sizeof(PoseJob) == 32 && sizeof(lmx_pose_refine_t) == 136 && sizeof(pr::Record) == sizeof(lmx_pose_refine_t), "layouts the kernel relies on");
static_assert(offsetof(pr::Record, rms_first_mm) == offsetof(lmx_pose_refine_t, rms_first_mm) && offsetof(pr::Record, status) == offsetof(lmx_pose_refine_t, status),
              "pr::Record is lmx_pose_refine_t");
static_assert(sizeof(pr::Stage) == sizeof(lmx_pose_refine_stage) && offsetof(pr::Stage, stride) == offsetof(lmx_pose_refine_stage, stride) && (int)LMX_POSE_MAX_STAGES == pr::kMaxStages,
              "pr::Stage is lmx_pose_refine_stage");

// Every crop pixel t != 0 once, f(i, j, t), spread over the workgroup the way diff_walk spreads them: lanes along the rows, one aligned
// 16-byte vector each, a narrow crop's rows packed into a wave, waves taking rows (groups of rows) in turn.
template <typename F>
__device__ __forceinline__ void crop_pixels(const DepthCrop& c, int lane, int wave, F&& f) {
  const int vpr = c.pitch / dv::kPitchAlign;
  const int lanes_per_row = vpr < dv::kWalkLanes ? vpr : dv::kWalkLanes;
  const int rows_per_pass = dv::kWalkLanes / lanes_per_row;
  const int sub = lane / lanes_per_row, v0 = lane - sub * lanes_per_row;
  for (int row0 = wave * rows_per_pass; row0 < c.h; row0 += 4 * rows_per_pass) {
    const int i = row0 + sub;
    if (sub >= rows_per_pass || i >= c.h) continue;
    const uint16_t* trow = c.data + (size_t)i * c.pitch;
    for (int v = v0; v < vpr; v += lanes_per_row) {
      const int col0 = v * dv::kPitchAlign;
      const uint4 q = load_global_16(trow + col0);    // past w: the padding, zeros
      const unsigned long long lo = q.x | ((unsigned long long)q.y << 32), hi = q.z | ((unsigned long long)q.w << 32);
#pragma unroll 1
      for (int e = 0; e < dv::kPitchAlign; ++e) {   // one copy of f's code: a pixel's work is hundreds of instructions
        const uint16_t t = (uint16_t)((e < 4 ? lo : hi) >> (16 * (e & 3)));
        if (t != 0) f(i, col0 + e, t);
      }
    }
  }
}

// The first n of a lane's sums added up over the wave, lane 0's totals into the wave's row of `part`; then the barrier behind which any
// lane may add the four rows.
template <int ROW>
__device__ __forceinline__ void wave_sums_to_lds(const int64_t* a, int n, long long (*part)[ROW], int lane, int wave) {
#pragma unroll
  for (int k = 0; k < n; ++k) {   // n is a constant at every call: the sums stay in registers
    const long long v = wave_sum<long long>((long long)a[k]);
    if (lane == 0) part[wave][k] = v;
  }
  __syncthreads();
}

// The selected pixels of a stage of stride > 1 (lmx_pose_refine.hpp, SCHEDULE), each once, f(i, j, t): the lattice positions numbered row-major
// over ceil(h / stride) x ceil(w / stride), the 256 lanes striding over that index, one 2-byte load each (i < h, j < w <= pitch: inside the
// crop).  crop_pixels would leave all but one lane in `stride` and all but one row in `stride` idle: a pass would cost what a full one costs.
// (ox, oy): where the lattice starts.  (0, 0) for a stored crop; a rough pose's crop is the silhouette box of its render, which lies at
// (ox, oy) inside the window the kernel walks (nothing but zeros lies in front of it).  Clamped into the crop: no index leaves it.
template <typename F>
__device__ __forceinline__ void lattice_pixels(const DepthCrop& c, int stride, int ox, int oy, int tid, F&& f) {
  const int shift = 31 - __builtin_clz(stride);   // 1, 2 or 3
  ox = ox < 0 ? 0 : ox > c.w ? c.w : ox;
  oy = oy < 0 ? 0 : oy > c.h ? c.h : oy;
  const int cols = (c.w - ox + stride - 1) >> shift, rows = (c.h - oy + stride - 1) >> shift;
  const int total = rows * cols;                  // at most 2^26
#pragma unroll 1
  for (int p = tid; p < total; p += 256) {
    const int li = p / cols, lj = p - li * cols;
    const int i = oy + (li << shift), j = ox + (lj << shift);
    const uint16_t t = c.data[(size_t)i * c.pitch + j];
    if (t != 0) f(i, j, t);
  }
}

// A value every lane holds alike, told to the compiler as that: scalar registers.
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// One 256-lane workgroup per job, every pass of every stage of it in this one launch.  A pass: each lane walks its crop pixels under the
// pose in LDS (pr::pass_pixel_rad: projection, the window of scene reads under the in-image predicate, the pair, its 17 integer terms), wave
// shuffles, LDS across the four waves; lane 0 adds them, solves, updates (pr::after_pass_staged) and leaves the next pose, its centre and
// "the stage of the next pass, plus one" (0: none) in LDS; a barrier; the next pass.  The stage's parameters are read from the schedule
// (a kernel argument) under that workgroup-uniform index: scalar loads, no vector registers.  A stage of stride 1 walks with crop_pixels,
// any other with lattice_pixels.  Integer sums: the result does not depend on which lane took which pixel.  No atomics, no workgroup
// waits for another.  What is no job (template or frame outside the tables) or has an empty crop gets a zeroed record before any barrier.
// dbg (null outside the test hook): the sums of job 0's passes, one row of 17 per pass in the order they ran.
// PLANE (lmx_pose_refine.hpp, PLANE; launched only when a stage in force has a point_shift >= 0, K): whether a stage is a plane stage is a
// workgroup-uniform branch.  A -1 stage runs the 17-sum pass above; a plane stage keeps 46 int64 sums per lane (the 17 and the 29), reads
// the chosen candidate's stored normal from `normals` (the scene's, [frame][H][W], made ready on the launch stream by scene_normals_on),
// reduces all 46 the same way and lane 0 takes solve_plane's step.  Its dbg rows are 46 wide, the 29 of a -1 stage's row left alone.
// Without PLANE neither `normals` nor K is read and the code is what it was before the parameter existed.
// pose_refine_body is that workgroup's work on one job and its record `out` (dbg: null, or where this job's sums go), shared by
// k_pose_refine, k_pose_refine_clusters and k_rough_refine_clusters; forceinline: each kernel gets its own copy of the LDS arrays.
template <bool PLANE>
__device__ __forceinline__ void pose_refine_body(const DepthCrop* __restrict__ crops, int32_t count, const PoseJob job, const uint16_t* __restrict__ scene,
                                                 int32_t n_frames, int W, int H, const pr::Params& P, const pr::Schedule& S, lmx_pose_refine_t* __restrict__ out,
                                                 long long* __restrict__ dbg, const nv::Packed* __restrict__ normals, const pr::PlaneShifts& K) {
  constexpr int ROW = PLANE ? pr::kAllSums : pr::kSums;
  __shared__ long long s_part[4][ROW];
  __shared__ pr::Pose s_pose;
  __shared__ double s_c[3];
  __shared__ long long s_C[3];
  __shared__ int s_more;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool is_job = job.template_id >= 0 && job.template_id < count && job.frame >= 0 && job.frame < n_frames;
  const DepthCrop c = is_job ? crops[job.template_id] : DepthCrop{nullptr, 0, 0, 0, 0};
  if (c.w <= 0 || c.h <= 0) {
    store_zero_record(out, tid);
    return;
  }
  const uint16_t* frame = scene + (size_t)job.frame * H * W;
  // lane 0's own: the record, the pose it advances, the control state
  pr::Record rec;
  pr::Pose pose0;
  pr::Control ctl = {0};
  pr::StagedControl sc = {0, 0, 0};
  double m0[3] = {0.0, 0.0, 0.0};

  int64_t a[ROW];
  for (int k = 0; k < pr::kSums; ++k) a[k] = 0;
  crop_pixels(c, lane, wave, [&](int i, int j, uint16_t t) {
    int32_t X = 0, Y = 0;
    const bool met = dv::scene_row(job.y, i, H, &Y) && dv::scene_col(job.x, j, W, &X);
    const uint16_t s = met ? frame[(size_t)Y * W + X] : (uint16_t)0;   // read only inside the image
    pr::place_pixel(job.rect_x, job.rect_y, i, j, t, X, Y, s, a);
  });
  wave_sums_to_lds(a, pr::kPlaceSums, s_part, lane, wave);
  if (tid == 0) {
    int64_t place[pr::kPlaceSums];
    for (int k = 0; k < pr::kPlaceSums; ++k) place[k] = s_part[0][k] + s_part[1][k] + s_part[2][k] + s_part[3][k];
    const bool more = pr::placement(P, place, m0, &pose0, &rec, &ctl);
    if (more) {
      int64_t C[3];
      pr::enter_stage(S, 0, &rec, &sc);
      pr::centre_of(pose0, m0, s_c, C);
      s_pose = pose0;
      for (int k = 0; k < 3; ++k) s_C[k] = C[k];
    } else {
      *reinterpret_cast<pr::Record*>(out) = rec;
    }
    s_more = more;
  }
  __syncthreads();
  if (!s_more) return;
  const pr::Inverse im = pr::inverse_of(P.model), is = pr::inverse_of(P.scene);
  int32_t stage = 0;
  for (int32_t pass = 0; pass <= pr::kMaxStages * pr::kMaxIterations; ++pass) {   // after_pass_staged ends it after schedule_passes(S) passes at the latest
    const pr::Stage& st = S.stage[stage];
    const int64_t dmax = uniform_i64(pr::dist_ticks(st.max_dist_mm));
    const int32_t radius = st.search_radius, stride = st.stride;
    const pr::Pose pose = s_pose;
    const int64_t C[3] = {s_C[0], s_C[1], s_C[2]};
    const bool plane = PLANE && K.shift[stage] >= 0;   // workgroup-uniform
    if (plane) {
      for (int q = 0; q < ROW; ++q) a[q] = 0;
      const nv::Packed* nframe = normals + (size_t)job.frame * H * W;
      auto pixel = [&](int i, int j, uint16_t t) {
        pr::pass_pixel_plane_rad(P, radius, im, is, pose, C, dmax, job.rect_x, job.rect_y, i, j, t, frame, nframe, W, H, (size_t)W, a, a + pr::kSums);
      };
      if (stride == 1) crop_pixels(c, lane, wave, pixel);
      else lattice_pixels(c, stride, job.lat_x, job.lat_y, tid, pixel);
      wave_sums_to_lds(a, ROW, s_part, lane, wave);
    } else {
      for (int q = 0; q < pr::kSums; ++q) a[q] = 0;
      auto pixel = [&](int i, int j, uint16_t t) {
        pr::pass_pixel_rad(P, radius, im, is, pose, C, dmax, job.rect_x, job.rect_y, i, j, t, frame, W, H, (size_t)W, a);
      };
      if (stride == 1) crop_pixels(c, lane, wave, pixel);
      else lattice_pixels(c, stride, job.lat_x, job.lat_y, tid, pixel);
      wave_sums_to_lds(a, pr::kSums, s_part, lane, wave);
    }
    if (tid == 0) {
      int64_t total[ROW];
      for (int q = 0; q < pr::kSums; ++q) total[q] = s_part[0][q] + s_part[1][q] + s_part[2][q] + s_part[3][q];
      if (plane)
        for (int q = pr::kSums; q < ROW; ++q) total[q] = s_part[0][q] + s_part[1][q] + s_part[2][q] + s_part[3][q];
      if (dbg) {
        for (int q = 0; q < pr::kSums; ++q) dbg[(size_t)pass * ROW + q] = total[q];
        if (plane)
          for (int q = pr::kSums; q < ROW; ++q) dbg[(size_t)pass * ROW + q] = total[q];
      }
      const double cc[3] = {s_c[0], s_c[1], s_c[2]};
      const bool more = PLANE ? pr::after_pass_plane(P, S, &K, total, total + pr::kSums, cc, &pose0, &rec, &sc) : pr::after_pass_staged(P, S, total, cc, &pose0, &rec, &sc);
      if (more) {
        int64_t Cn[3];
        pr::centre_of(pose0, m0, s_c, Cn);
        s_pose = pose0;
        for (int q = 0; q < 3; ++q) s_C[q] = Cn[q];
      } else {
        *reinterpret_cast<pr::Record*>(out) = rec;
      }
      s_more = more ? sc.stage + 1 : 0;
    }
    __syncthreads();
    const int next = __builtin_amdgcn_readfirstlane(s_more);
    if (!next) return;
    stage = next - 1;
  }
}

template <bool PLANE>
__global__ __launch_bounds__(256) void k_pose_refine(const DepthCrop* __restrict__ crops, int32_t count, const PoseJob* __restrict__ jobs,
                                                     const uint16_t* __restrict__ scene, int32_t n_frames, int W, int H, const pr::Params P, const pr::Schedule S,
                                                     lmx_pose_refine_t* __restrict__ out, long long* __restrict__ dbg, const nv::Packed* __restrict__ normals,
                                                     const pr::PlaneShifts K) {
  pose_refine_body<PLANE>(crops, count, jobs[blockIdx.x], scene, n_frames, W, H, P, S, &out[blockIdx.x], blockIdx.x == 0 ? dbg : nullptr, normals, K);
}

// ---- pose verification (lmx_pose_verify_matches; arithmetic: lmx_pose_verify.hpp) ---------------------------------------------------------------------
struct VerifyJob { int32_t template_id, frame, rect_x, rect_y; double R[9], t_mm[3]; };   // frame: as DepthJob's
static_assert(sizeof(VerifyJob) == 112 && sizeof(lmx_pose_verify_t) == 48 && sizeof(pv::Record) == sizeof(lmx_pose_verify_t), "layouts the kernel relies on");
static_assert(offsetof(pv::Record, n_model) == offsetof(lmx_pose_verify_t, n_model) && offsetof(pv::Record, status) == offsetof(lmx_pose_verify_t, status) &&
                  offsetof(pv::Record, roi) == offsetof(lmx_pose_verify_t, roi),
              "pv::Record is lmx_pose_verify_t");

// One 256-lane workgroup per job, four phases in one launch with a barrier between them:
//   1  the crop walk of k_pose_refine under the job's pose: each lane's extent of keys and projections and its two counts (pv::bounds_pixel),
//      wave shuffles, LDS across the four waves; lane 0 merges them and leaves the grid and the ROI in LDS (pv::grid_of), or the final
//      record when there is nothing to test or the grid exceeds the bitmap
//   2  the bitmap's ceil(cells / 32) words cleared
//   3  the ROI's pixels in raster order over the workgroup, so that a wave reads runs of neighbouring uint16 of a scene row; every read lies
//      inside the image (the ROI is clipped to it); a pixel that marks a cell sets its bit with an LDS atomic OR
//   4  the crop walk again, every point recomputed from phase 1's expressions (no per-point state is kept: a crop holds far more points
//      than the workgroup has lanes), its bit tested
// The counts are integer sums and marking is idempotent: the result does not depend on which lane took which pixel.  What is no job
// (template or frame outside the tables) or has an empty crop gets a zeroed record before any barrier.
// pose_verify_body is that workgroup's work on one job and its record `out`, shared by k_pose_verify and k_pose_verify_clusters.  job_R /
// job_t: the pose, in device memory.  *rec0: lane 0's copy of the record it stored (zeros where the first lanes store zeros), for a caller
// that goes on from it.
__device__ __forceinline__ void pose_verify_body(const DepthCrop* __restrict__ crops, int32_t count, int32_t template_id, int32_t frame_id, int32_t rect_x,
                                                 int32_t rect_y, const double* __restrict__ job_R, const double* __restrict__ job_t,
                                                 const uint16_t* __restrict__ scene, int32_t n_frames, int W, int H, const pv::Params& P,
                                                 lmx_pose_verify_t* __restrict__ out, pv::Record* rec0) {
  __shared__ uint32_t s_bits[pv::kBitmapWords];
  static_assert(sizeof(s_bits) == 32768 && (size_t)pv::kMaxCells == 8 * sizeof(s_bits), "kMaxCells is the bitmap in LDS");
  __shared__ pv::Bounds s_bounds[4];
  __shared__ pv::Grid s_grid;
  __shared__ int s_count[8];
  __shared__ int s_more;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool is_job = template_id >= 0 && template_id < count && frame_id >= 0 && frame_id < n_frames;
  const DepthCrop c = is_job ? crops[template_id] : DepthCrop{nullptr, 0, 0, 0, 0};
  if (c.w <= 0 || c.h <= 0) {
    store_zero_record(out, tid);
    *rec0 = pv::Record{0.0, 0, 0, 0, 0, 0, pv::NONE, {0, 0, 0, 0}};
    return;
  }
  const uint16_t* frame = scene + (size_t)frame_id * H * W;
  double R[9], t_mm[3];
  for (int k = 0; k < 9; ++k) R[k] = job_R[k];
  for (int k = 0; k < 3; ++k) t_mm[k] = job_t[k];
  const int32_t vt = pv::voxel_ticks(P);
  const pr::Inverse im = pr::inverse_of(P.model), is = pr::inverse_of(P.scene);
  pv::Record& rec = *rec0;   // lane 0's own

  // 1
  pv::Bounds b;
  pv::bounds_init(&b);
  crop_pixels(c, lane, wave, [&](int i, int j, uint16_t t) { pv::bounds_pixel(P, im, R, t_mm, vt, rect_x, rect_y, i, j, t, &b); });
  for (int k = 0; k < 3; ++k) { b.lo[k] = wave_min(b.lo[k]); b.hi[k] = wave_max(b.hi[k]); }
  b.xmin = wave_min(b.xmin); b.ymin = wave_min(b.ymin);
  b.xmax = wave_max(b.xmax); b.ymax = wave_max(b.ymax);
  b.n_model = wave_sum(b.n_model); b.n_tested = wave_sum(b.n_tested);
  if (lane == 0) s_bounds[wave] = b;
  __syncthreads();
  if (tid == 0) {
    pv::Bounds all = s_bounds[0];
    for (int k = 1; k < 4; ++k) pv::bounds_merge(&all, s_bounds[k]);
    pv::Grid g;
    const bool more = pv::grid_of(P, all, W, H, &g, &rec);
    if (more) s_grid = g;
    else *reinterpret_cast<pv::Record*>(out) = rec;
    s_more = more;
  }
  __syncthreads();
  if (!s_more) return;
  const pv::Grid g = s_grid;

  // 2
  const int words = pv::bitmap_words(g);   // <= kBitmapWords: grid_of refused more cells
  for (int k = tid; k < words; k += 256) s_bits[k] = 0;
  __syncthreads();

  // 3
  int n_scene = 0;
  const int n_roi = g.roi_w * g.roi_h;   // at most W * H, which the host keeps inside an int32
  for (int q = tid; q < n_roi; q += 256) {
    const int row = q / g.roi_w, X = g.x0 + (q - row * g.roi_w), Y = g.y0 + row;
    const uint16_t s = frame[(size_t)Y * W + X];
    if (s == 0) continue;
    const int32_t cell = pv::scene_cell(P, is, g, vt, X, Y, s);
    if (cell < 0) continue;
    atomicOr(&s_bits[cell >> 5], 1u << (cell & 31));
    n_scene += 1;
  }
  __syncthreads();

  // 4
  int n_occupied = 0;
  crop_pixels(c, lane, wave, [&](int i, int j, uint16_t t) {
    const int32_t cell = pv::model_cell(P, im, R, t_mm, g, vt, rect_x, rect_y, i, j, t);
    if (cell >= 0) n_occupied += (int)((s_bits[cell >> 5] >> (cell & 31)) & 1u);
  });
  n_scene = wave_sum(n_scene);
  n_occupied = wave_sum(n_occupied);
  if (lane == 0) { s_count[wave] = n_scene; s_count[4 + wave] = n_occupied; }
  __syncthreads();
  if (tid == 0) {
    pv::finish(s_count[0] + s_count[1] + s_count[2] + s_count[3], s_count[4] + s_count[5] + s_count[6] + s_count[7], &rec);
    *reinterpret_cast<pv::Record*>(out) = rec;
  }
}

__global__ __launch_bounds__(256) void k_pose_verify(const DepthCrop* __restrict__ crops, int32_t count, const VerifyJob* __restrict__ jobs,
                                                     const uint16_t* __restrict__ scene, int32_t n_frames, int W, int H, const pv::Params P,
                                                     lmx_pose_verify_t* __restrict__ out) {
  const VerifyJob* job = jobs + blockIdx.x;
  pv::Record rec;
  pose_verify_body(crops, count, job->template_id, job->frame, job->rect_x, job->rect_y, job->R, job->t_mm, scene, n_frames, W, H, P, &out[blockIdx.x], &rec);
}

// What the two cluster-chain verify kernels do for a slot once they know whether it has a job: every lane reads the pose's status, R and
// t_mm from *pose; a slot without a job, a pose of status LMX_POSE_NONE and one that pv::check_pose refuses (the host call refuses the
// whole call there; here: a flag) get the zeroed record, the others pose_verify_body.  Lane 0 then has the record it stored: the keep
// decision, and the header's three counters by vector atomic adds.
__device__ __forceinline__ void verify_tail(bool has_job, const DepthCrop* crops, int32_t count, int32_t template_id, int32_t frame, int32_t rect_x, int32_t rect_y,
                                            const uint16_t* scene, int32_t n_frames, int W, int H, const pv::Params& P, const lmx_pose_refine_t* pose,
                                            lmx_pose_verify_t* check, uint8_t* keep, double keep_thresh, uint32_t* chain_header) {
  const int tid = threadIdx.x;
  const bool refined = has_job && pose->status != LMX_POSE_NONE;
  const bool pose_ok = refined && pv::check_pose(pose->R, pose->t_mm) == nullptr;
  pv::Record rec = {0.0, 0, 0, 0, 0, 0, pv::NONE, {0, 0, 0, 0}};
  if (pose_ok) pose_verify_body(crops, count, template_id, frame, rect_x, rect_y, pose->R, pose->t_mm, scene, n_frames, W, H, P, check, &rec);
  else store_zero_record(check, tid);
  if (tid == 0) {
    const bool kept = pv::keep(rec, keep_thresh);
    *keep = kept ? 1 : 0;
    if (refined) atomicAdd(&chain_header[pc::C_REFINED], 1u);
    if (refined && !pose_ok) atomicOr(&chain_header[pc::C_FLAGS], (uint32_t)pc::FLAG_POSE);
    if (rec.status == pv::OK) atomicAdd(&chain_header[pc::C_VERIFIED], 1u);
    if (kept) atomicAdd(&chain_header[pc::C_KEPT], 1u);
  }
}

// ---- both stages on exported clusters (lmx_pose_chain_on; the decisions: lmx_pose_chain.hpp) -----------------------------------------------------------
static_assert(sizeof(pc::Match) == sizeof(lmx_match_t) && offsetof(pc::Match, template_id) == offsetof(lmx_match_t, template_id) &&
                  sizeof(pc::Cluster) == sizeof(lmx_cluster_t) && offsetof(pc::Cluster, member_begin) == offsetof(lmx_cluster_t, member_begin),
              "pc::Match is lmx_match_t, pc::Cluster is lmx_cluster_t");
struct ChainArgs {
  pc::Lists L;                 // what an export wrote, device memory
  pc::Table T;                 // rects and class_base in device memory
  const DepthCrop* crops;
  const uint16_t* scene;       // L.n_frames frames of W x H
  int32_t W, H;
  uint32_t* chain_header;      // [pc::C_WORDS], zeroed in front of the first kernel
  int32_t* leaders;
  lmx_pose_refine_t* poses;
  lmx_pose_verify_t* checks;
  uint8_t* keep;
  double keep_thresh;
};

// Slot k as the 64 lanes of one wave decide it (every lane returns the same): the frames and the members spread over the lanes, the two
// reductions by shuffles, everything else lmx_pose_chain.hpp.  The branches of slot_from_claims depend on k and on device memory alone,
// so the wave stays together through the shuffles.
__device__ __forceinline__ pc::Slot chain_slot(const ChainArgs& a, uint32_t k, int lane, bool pick, int32_t leader_in) {
  int32_t claims = 0, first = INT32_MAX;
  for (int32_t f = lane; f < a.L.n_frames; f += pc::kLanes)
    if (pc::frame_claims(a.L, f, k)) { claims += 1; first = f < first ? f : first; }
  claims = __shfl(wave_sum(claims), 0, 64);
  first = __shfl(wave_min(first), 0, 64);
  return pc::slot_from_claims(a.L, a.T, k, claims, first, pick, leader_in, [&](const pc::Frame& fr, const pc::Cluster& c) {
    pc::Best b = pc::best_of_lane(a.L, fr, c, lane, pc::kLanes);
    for (int off = 32; off > 0; off >>= 1) {
      pc::Best o;
      o.key = __shfl_down(b.key, off, 64); o.pos = __shfl_down(b.pos, off, 64); o.bad = __shfl_down(b.bad, off, 64);
      b = pc::best_merge(b, o);   // a total order: whatever the upper lanes merge in, lane 0 ends with the wave's best
    }
    b.key = __shfl(b.key, 0, 64); b.pos = __shfl(b.pos, 0, 64); b.bad = __shfl(b.bad, 0, 64);
    return b;
  });
}

// The slot wave 0 left in LDS, told to the compiler as what it is: the same in every lane (scalar registers, none of the body's vector ones).
__device__ __forceinline__ pc::Slot uniform_slot(const pc::Slot& v) {
  pc::Slot s;
  s.state = __builtin_amdgcn_readfirstlane(v.state); s.flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.flags);
  s.leader = __builtin_amdgcn_readfirstlane(v.leader); s.frame = __builtin_amdgcn_readfirstlane(v.frame);
  s.x = __builtin_amdgcn_readfirstlane(v.x); s.y = __builtin_amdgcn_readfirstlane(v.y); s.template_id = __builtin_amdgcn_readfirstlane(v.template_id);
  s.rect_x = __builtin_amdgcn_readfirstlane(v.rect_x); s.rect_y = __builtin_amdgcn_readfirstlane(v.rect_y);
  return s;
}

// One 256-lane workgroup per cluster slot, a grid of cap_clusters: the count is in device memory, and a workgroup at or above n_live
// leaves at once without a store.  Wave 0 decides the slot and leaves it in LDS; one barrier; then either the zeroed record (a dead slot,
// a broken list, no job) or k_pose_refine's body on the leader's job.  Workgroup 0 also reports n_live and the header's flag; a slot's
// flags go to chain_header[1] by a vector atomic OR of lane 0.  waves_per_eu(2): the body sits at 247 vector registers; without the
// attribute the prologue's scalar spills take the kernel a few registers past 256 and to half of k_pose_refine's occupancy.
template <bool PLANE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PLANE ? 1 : 2))) void k_pose_refine_clusters(const ChainArgs a, const pr::Params P, const pr::Schedule S,
                                                                                                      const nv::Packed* __restrict__ normals, const pr::PlaneShifts K) {
  __shared__ pc::Slot s_slot;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t k = blockIdx.x, n_live = pc::n_live(a.L);
  if (k == 0 && tid == 0) {
    a.chain_header[pc::C_LIVE] = n_live;
    const uint32_t hf = pc::header_flags(a.L);
    if (hf) atomicOr(&a.chain_header[pc::C_FLAGS], hf);
  }
  if (k >= n_live) return;
  if (wave == 0) {
    const pc::Slot s = chain_slot(a, k, lane, true, -1);
    if (lane == 0) s_slot = s;
  }
  __syncthreads();
  const pc::Slot s = uniform_slot(s_slot);
  if (tid == 0) {
    a.leaders[k] = s.leader;
    if (s.flags) atomicOr(&a.chain_header[pc::C_FLAGS], s.flags);
  }
  if (s.state != pc::JOB) {
    store_zero_record(&a.poses[k], tid);
    return;
  }
  const PoseJob job = {s.x, s.y, s.template_id, s.frame, s.rect_x, s.rect_y, 0, 0};
  pose_refine_body<PLANE>(a.crops, a.T.count, job, a.scene, a.L.n_frames, a.W, a.H, P, S, &a.poses[k], nullptr, normals, K);
}

// The same grid behind it.  Wave 0 decides the slot again from leaders[k] (the job is not kept between the kernels: a match, a frame and a
// rect are cheaper to read again than to store), then verify_tail.
__global__ __launch_bounds__(256) void k_pose_verify_clusters(const ChainArgs a, const pv::Params P) {
  __shared__ pc::Slot s_slot;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t k = blockIdx.x;
  if (k >= pc::n_live(a.L)) return;
  if (wave == 0) {
    const pc::Slot s = chain_slot(a, k, lane, false, a.leaders[k]);
    if (lane == 0) s_slot = s;
  }
  __syncthreads();
  const pc::Slot s = uniform_slot(s_slot);
  verify_tail(s.state == pc::JOB, a.crops, a.T.count, s.template_id, s.frame, s.rect_x, s.rect_y, a.scene, a.L.n_frames, a.W, a.H, P, &a.poses[k], &a.checks[k],
              &a.keep[k], a.keep_thresh, a.chain_header);
}

// ---- both stages behind the rough pose stage (lmx_rough_pose_chain_on; lmx_rough.hip leaves a job and a crop table entry per slot) -------------------
static_assert(sizeof(rp::CropEntry) == sizeof(DepthCrop) && offsetof(rp::CropEntry, w) == offsetof(DepthCrop, w) && offsetof(rp::CropEntry, pitch) == offsetof(DepthCrop, pitch),
              "rp::CropEntry is DepthCrop");
static_assert(sizeof(rp::Record) == sizeof(lmx_rough_pose_t) && offsetof(rp::Record, x) == offsetof(lmx_rough_pose_t, x) &&
                  offsetof(rp::Record, rect) == offsetof(lmx_rough_pose_t, rect) && offsetof(rp::Record, status) == offsetof(lmx_rough_pose_t, status) &&
                  alignof(lmx_rough_pose_t) == 8,
              "rp::Record is lmx_rough_pose_t");
struct RoughChainArgs {
  const uint32_t* header;      // the export's
  uint64_t cap_clusters;
  const rp::Job* jobs;         // the model's, [cap_slots]
  const DepthCrop* crops;      // the model's, [cap_slots]: slot k's render is template k
  int32_t cap_slots;
  const uint16_t* scene;
  int32_t n_frames, W, H;
  uint32_t* chain_header;
  lmx_pose_refine_t* poses;
  lmx_pose_verify_t* checks;
  uint8_t* keep;
  double keep_thresh;
};

// k_pose_refine_clusters' grid and body; the prologue is two loads: k_rough_finish decided the slot and left its job.  The job's fields
// are told to the compiler as uniform, as uniform_slot does.  247 vector registers, 106 scalar, 592 bytes of scratch per lane (the body's
// local arrays, as in k_pose_refine: 247, 106, 592), 2 waves per SIMD as k_pose_refine and k_pose_refine_clusters (249, 106, 592);
// the figures before the stage loop are in profiles/pose_refine_staged.txt.
// k_rough_verify_clusters: 67 vector registers, 106 scalar, no scratch, 4 waves per SIMD, as k_pose_verify_clusters.
template <bool PLANE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PLANE ? 1 : 2))) void k_rough_refine_clusters(const RoughChainArgs a, const pr::Params P, const pr::Schedule S,
                                                                                                       const nv::Packed* __restrict__ normals, const pr::PlaneShifts K) {
  const uint32_t k = blockIdx.x;
  if (k >= pc::n_live(a.header, a.cap_clusters)) return;
  const rp::Job* j = a.jobs + k;
  const int tid = threadIdx.x;
  if (!__builtin_amdgcn_readfirstlane(j->run)) {
    store_zero_record(&a.poses[k], tid);
    return;
  }
  const PoseJob job = {__builtin_amdgcn_readfirstlane(j->x), __builtin_amdgcn_readfirstlane(j->y), (int32_t)k, __builtin_amdgcn_readfirstlane(j->frame),
                       __builtin_amdgcn_readfirstlane(j->rect_x), __builtin_amdgcn_readfirstlane(j->rect_y), __builtin_amdgcn_readfirstlane(j->lat_x),
                       __builtin_amdgcn_readfirstlane(j->lat_y)};
  pose_refine_body<PLANE>(a.crops, a.cap_slots, job, a.scene, a.n_frames, a.W, a.H, P, S, &a.poses[k], nullptr, normals, K);
}

// k_pose_verify_clusters behind it, on the same job.
__global__ __launch_bounds__(256) void k_rough_verify_clusters(const RoughChainArgs a, const pv::Params P) {
  const uint32_t k = blockIdx.x;
  if (k >= pc::n_live(a.header, a.cap_clusters)) return;
  const rp::Job* j = a.jobs + k;
  verify_tail(__builtin_amdgcn_readfirstlane(j->run) != 0, a.crops, a.cap_slots, (int32_t)k, __builtin_amdgcn_readfirstlane(j->frame),
              __builtin_amdgcn_readfirstlane(j->rect_x), __builtin_amdgcn_readfirstlane(j->rect_y), a.scene, a.n_frames, a.W, a.H, P, &a.poses[k], &a.checks[k],
              &a.keep[k], a.keep_thresh, a.chain_header);
}

}  // namespace
}  // namespace lmx

struct lmx_depth_templates {
  int32_t device = 0;
  std::mutex m;
  std::vector<lmx::DepthCrop> table;     // host copy; the addresses are device addresses
  std::vector<int32_t> rects;            // [n][4]
  std::vector<void*> chunks;
  size_t atlas_bytes = 0;
  // what a call needs on the device, created on first use
  hipStream_t s = nullptr;
  lmx::DepthCrop* d_table = nullptr;
  uint16_t *d_scene = nullptr, *h_scene = nullptr;
  size_t scene_cap = 0;                  // bytes
  // the scene lmx_depth_templates_upload_scene left on the device (scene_frames 0: none); scene_ready is recorded behind its copies
  int32_t scene_frames = 0, scene_W = 0, scene_H = 0;
  hipEvent_t scene_ready = nullptr;
  hipEvent_t scene_src_ready = nullptr;  // lmx_depth_templates_upload_scene_device: recorded on the caller's stream in front of the copies
  bool scene_pending = false;            // scene_ready has been recorded and h_scene may still be read by a copy
  lmx::DepthJob *d_jobs = nullptr, *h_jobs = nullptr;
  lmx_depth_diff_t *d_out = nullptr, *h_out = nullptr;
  size_t jobs_cap = 0, out_cap = 0;      // entries
  lmx::PoseJob *d_pjobs = nullptr, *h_pjobs = nullptr;   // lmx_pose_refine_matches: its jobs and records, as d_jobs / d_out
  lmx_pose_refine_t *d_pout = nullptr, *h_pout = nullptr;
  size_t pjobs_cap = 0, pout_cap = 0;
  // lmx_depth_templates_set_refine_schedule (n_stages 0: none).  A call reads it under `m` and hands it to its kernel by value
  lmx::pr::Schedule schedule = {0, 0, {}};
  lmx::pr::Schedule schedule_for(const lmx::pr::Params& P) const { return schedule.n_stages > 0 ? schedule : lmx::pr::single_stage(P); }
  // lmx_depth_templates_set_refine_plane: entry s is stage s's point_shift of whatever schedule is in force (a call without one is stage 0),
  // -1 beyond plane_stages; read under `m` like the schedule and handed to the kernel by value
  lmx::pr::PlaneShifts plane = lmx::pr::kNoPlane;
  int32_t plane_stages = 0;
  // does a call under schedule S run the PLANE kernels?
  bool plane_for(const lmx::pr::Schedule& S) const { return lmx::pr::any_plane(plane, S.n_stages); }
  lmx::VerifyJob *d_vjobs = nullptr, *h_vjobs = nullptr;   // lmx_pose_verify_matches: the same pair
  lmx_pose_verify_t *d_vout = nullptr, *h_vout = nullptr;
  size_t vjobs_cap = 0, vout_cap = 0;
  std::vector<uint32_t> sel;             // scratch of a call: the matches it computes
  std::vector<int32_t> sel_slot;         // scratch of a call: the uploaded frame of each of them
  std::vector<int32_t> slot;             // scratch of a call: frame -> uploaded frame, or -1
  // the normal term (lmx_depth_templates_enable_normals): nothing below is allocated, and no kernel of it launched, before that call
  bool normals_on = false;
  bool ncrops_ready = false;             // the crops' normals for nparams are on the device (an object without pixels defers them)
  lmx::nv::Params nparams = {0.0f, 0.0f, 0, 0};
  lmx::nv::Packed* d_ncrops = nullptr;   // every crop's normals back to back, each [h][pitch] as its depth crop (8 bytes for 2)
  std::vector<lmx::nv::Packed*> ntable;  // host copy of d_ntable: where template i's normals start (null for an empty crop)
  lmx::nv::Packed** d_ntable = nullptr;
  uint32_t* d_angle = nullptr;           // the chord -> angle table, nv::kAngleTableSize entries
  lmx::nv::Packed* d_scene_normals = nullptr;   // [frames][H][W] next to d_scene, computed when first needed
  size_t scene_normals_cap = 0;          // bytes
  bool scene_normals_valid = false;      // they belong to the frames now in d_scene
  hipEvent_t normals_ready = nullptr;    // recorded behind the kernel that computed them (it may run on a caller's stream)
  lmx_normal_diff_t *d_nout = nullptr, *h_nout = nullptr;   // as d_out / h_out
  size_t nout_cap = 0;
  // the scene filter (lmx_depth_templates_set_scene_filter; lmx_scene_filter.hpp): nothing below is allocated, and no kernel of it launched,
  // before that call.  While filter_on, the pose stages read d_scene_filtered where they read d_scene otherwise (pose_scene_on)
  bool filter_on = false;
  lmx::sf::Params fparams = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0, 0};
  uint16_t* d_scene_filtered = nullptr;     // [frames][H][W] next to d_scene, computed when first needed
  uint32_t* d_scene_score = nullptr;        // [frames][H][W]: the score map between the two kernels
  lmx::sf::Info* d_filter_info = nullptr;   // [frames]
  size_t scene_filtered_cap = 0, filter_info_cap = 0;   // pixels, frames
  bool scene_filtered_valid = false;        // they belong to the frames now in d_scene and to fparams
  hipEvent_t filtered_ready = nullptr;      // recorded behind the kernels that computed them
  // lmx_ctx_export_clusters_on: its walk reads the table, the crops, the scene and the normals on a context's export stream and nobody
  // waits for it on the host.  export_read is recorded behind each such walk (an export's stream waits for the previous record first, so
  // the last record stands behind all of them); whoever changes what the walk reads waits for it: wait_export_reads() on the host,
  // lmx_depth_templates_upload_scene_device on the device
  hipEvent_t export_read = nullptr;
  bool export_read_pending = false;
  // lmx_pose_chain_on: its kernels run on `s` behind chain_src_ready (recorded on the caller's stream) and record export_read behind them, as
  // an export's walk does: they read the same things.  The rects of both stages and class_base in device memory, uploaded on the first
  // call and when they differ from the previous call's
  struct DevInts { std::vector<int32_t> host; int32_t* dev = nullptr; size_t cap = 0; };
  DevInts chain_rects_refine, chain_rects_verify, chain_base;
  hipEvent_t chain_src_ready = nullptr;
  int32_t walk_grid = 0;                 // workgroups of k_walk_records_dev; 0: not asked for yet (kWalkGridPerCU per compute unit)
  // lmx_depth_templates_set_profiling: a pair of events around each launch of the kernels below, read out by ..._kernel_time
  enum { PK_NORMAL_MAP_FRAMES, PK_VERIFY_DIFF_RECORDS, PK_VERIFY_DIFF, PK_DEPTH_DIFF_RECORDS, PK_WALK_RECORDS_DEV, PK_POSE_REFINE, PK_POSE_VERIFY, PK_POSE_REFINE_CLUSTERS,
         PK_POSE_VERIFY_CLUSTERS, PK_SCENE_FILTER_SCORE, PK_SCENE_FILTER_APPLY, PK_COUNT };
  struct ProfEvent { int kernel; hipEvent_t start, stop; };
  bool profiling = false;
  std::vector<ProfEvent> prof_pending;
  double prof_ms[PK_COUNT] = {};
  int64_t prof_launches[PK_COUNT] = {};
  // around a launch on stream `on`: begin returns the slot end takes (-1: profiling is off or an event could not be made)
  int prof_begin(int kernel, hipStream_t on) {
    if (!profiling) return -1;
    ProfEvent e{kernel, nullptr, nullptr};
    if (hipEventCreate(&e.start) != hipSuccess || hipEventCreate(&e.stop) != hipSuccess || hipEventRecord(e.start, on) != hipSuccess) {
      if (e.start) (void)hipEventDestroy(e.start);
      if (e.stop) (void)hipEventDestroy(e.stop);
      return -1;
    }
    prof_pending.push_back(e);
    return (int)prof_pending.size() - 1;
  }
  void prof_end(int slot, hipStream_t on) {
    if (slot >= 0) (void)hipEventRecord(prof_pending[(size_t)slot].stop, on);
  }
  void prof_drain() {
    for (const ProfEvent& e : prof_pending) {
      float ms = 0.0f;
      if (hipEventSynchronize(e.stop) == hipSuccess && hipEventElapsedTime(&ms, e.start, e.stop) == hipSuccess) { prof_ms[e.kernel] += ms; prof_launches[e.kernel] += 1; }
      (void)hipEventDestroy(e.start); (void)hipEventDestroy(e.stop);
    }
    prof_pending.clear();
  }

  lmx_status ensure_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { lmx::set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
    HIP_RETURN(hipSetDevice(device));
    if (!s) HIP_RETURN(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (!scene_ready) HIP_RETURN(hipEventCreateWithFlags(&scene_ready, hipEventDisableTiming));
    if (!d_table && !table.empty()) {
      HIP_RETURN(hipMalloc(&d_table, table.size() * sizeof(lmx::DepthCrop)));
      HIP_RETURN(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(lmx::DepthCrop), hipMemcpyHostToDevice, s));
      HIP_RETURN(hipStreamSynchronize(s));
    }
    return LMX_OK;
  }
  // Nothing an export queued still reads the crops, the table, the scene or the normals.
  lmx_status wait_export_reads() {
    if (export_read_pending) { HIP_RETURN(hipSetDevice(device)); HIP_RETURN(hipEventSynchronize(export_read)); export_read_pending = false; }
    return LMX_OK;
  }
  // The staging buffer is free again: the copies of the previous upload_scene have left it.
  lmx_status wait_scene_copies() {
    if (scene_pending) { HIP_RETURN(hipEventSynchronize(scene_ready)); scene_pending = false; }
    return LMX_OK;
  }
  // A call failed with copies of earlier frames possibly still queued: nothing may read the staging buffer once the call has returned, since
  // no event stands behind those copies for the next call to wait on.  The error already set is the one reported.
  void drain_after_error() { (void)hipStreamSynchronize(s); }
  lmx_status grow_scene(size_t bytes) {
    if (bytes <= scene_cap) return LMX_OK;
    HIP_RETURN(hipStreamSynchronize(s));     // nothing queued may still use the buffers that go
    if (lmx_status st = wait_export_reads()) return st;
    (void)hipFree(d_scene); (void)hipHostFree(h_scene);
    d_scene = h_scene = nullptr; scene_cap = 0;
    const size_t cap = bytes;
    HIP_RETURN(hipMalloc(&d_scene, cap));
    HIP_RETURN(hipHostMalloc(&h_scene, cap, hipHostMallocDefault));
    scene_cap = cap;
    return LMX_OK;
  }
  // a device array and its pinned twin hold at least n entries
  template <typename T>
  static lmx_status grow_pair(T*& d, T*& h, size_t& cap, size_t n) {
    if (n <= cap) return LMX_OK;
    (void)hipFree(d); (void)hipHostFree(h);
    d = h = nullptr; cap = 0;
    const size_t want = std::max(n, (size_t)1024);
    HIP_RETURN(hipMalloc(&d, want * sizeof(T)));
    HIP_RETURN(hipHostMalloc(&h, want * sizeof(T), hipHostMallocDefault));
    cap = want;
    return LMX_OK;
  }
  // Room for n jobs and their depth results; for their normal results only when a call asks (an object without normals never does).
  lmx_status grow_jobs(size_t n, bool normals) {
    if (lmx_status st = grow_pair(d_jobs, h_jobs, jobs_cap, n)) return st;
    if (lmx_status st = grow_pair(d_out, h_out, out_cap, n)) return st;
    return normals ? grow_pair(d_nout, h_nout, nout_cap, n) : LMX_OK;
  }
  // The normals of the first n_frames W x H frames of d_scene, on stream `on` (which already waits for the frames' copies, or is the
  // object's own stream that carries them); every later user waits for normals_ready.
  lmx_status compute_scene_normals(hipStream_t on, int32_t n_frames, int32_t W, int32_t H) {
    const size_t bytes = (size_t)W * H * (size_t)n_frames * sizeof(lmx::nv::Packed);
    if (bytes > scene_normals_cap) {     // every call that read the old buffer ended synchronised, but for an export's walk
      if (lmx_status st = wait_export_reads()) return st;
      (void)hipFree(d_scene_normals);
      d_scene_normals = nullptr; scene_normals_cap = 0;
      HIP_RETURN(hipMalloc(&d_scene_normals, bytes));
      scene_normals_cap = bytes;
    }
    const unsigned gx = (unsigned)std::min<size_t>(((size_t)W * H + 255) / 256, (size_t)lmx::nv::kFrameMapGridCap);
    const int pe = prof_begin(PK_NORMAL_MAP_FRAMES, on);
    hipLaunchKernelGGL(lmx::k_normal_map_frames, dim3(gx, (unsigned)n_frames), dim3(256), 0, on, d_scene, W, H, d_scene_normals, nparams);
    prof_end(pe, on);
    HIP_RETURN(hipGetLastError());
    HIP_RETURN(hipEventRecord(normals_ready, on));
    return LMX_OK;
  }
  // what every normal-scored call needs next to ensure_device(): the angle table and the event
  lmx_status ensure_normal_device() {
    if (!normals_ready) HIP_RETURN(hipEventCreateWithFlags(&normals_ready, hipEventDisableTiming));
    if (!d_angle) {
      std::vector<uint32_t> tab(lmx::nv::kAngleTableSize);
      lmx::nv::build_angle_table(tab.data());
      HIP_RETURN(hipMalloc(&d_angle, tab.size() * sizeof(uint32_t)));
      HIP_RETURN(hipMemcpyAsync(d_angle, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      HIP_RETURN(hipStreamSynchronize(s));   // tab goes when this returns
    }
    return LMX_OK;
  }
  // Stream `on` is about to read the normals of the n_frames W x H frames in d_scene: compute them there if nobody has (behind the scene's
  // copies: `behind_copies` is null when `on` is the stream that carries them), or wait for whoever did.
  lmx_status scene_normals_on(hipStream_t on, hipEvent_t behind_copies, int32_t n_frames, int32_t W, int32_t H) {
    if (scene_normals_valid) { HIP_RETURN(hipStreamWaitEvent(on, normals_ready, 0)); return LMX_OK; }
    if (behind_copies) HIP_RETURN(hipStreamWaitEvent(on, behind_copies, 0));
    if (lmx_status st = compute_scene_normals(on, n_frames, W, H)) return st;
    scene_normals_valid = true;
    return LMX_OK;
  }
  // A PLANE launch on stream `on` reads the scene's normals: as a normal-scored walk, but it needs neither the crops' normals nor the
  // angle table.  The setter saw enable_normals.
  lmx_status plane_normals_on(hipStream_t on, int32_t n_frames, int32_t W, int32_t H) {
    if (!normals_on) { lmx::set_error("a point_shift >= 0 is set and the normals are off: call lmx_depth_templates_enable_normals first"); return LMX_ERR_INVALID_ARG; }
    if (!normals_ready) HIP_RETURN(hipEventCreateWithFlags(&normals_ready, hipEventDisableTiming));
    return scene_normals_on(on, nullptr, n_frames, W, H);
  }
  // The filtered copies of the first n_frames W x H frames of d_scene under fparams, on stream `on` (which carries the frames' copies or
  // already waits for them); every later user waits for filtered_ready.  Nothing here waits on the host but a reallocation.
  lmx_status compute_scene_filtered(hipStream_t on, int32_t n_frames, int32_t W, int32_t H) {
    const size_t px = (size_t)W * H * (size_t)n_frames;
    if (px > scene_filtered_cap || (size_t)n_frames > filter_info_cap) {   // as the normals: every reader ended synchronised, but for a chain's kernels
      if (lmx_status st = wait_export_reads()) return st;
      (void)hipFree(d_scene_filtered); (void)hipFree(d_scene_score); (void)hipFree(d_filter_info);
      d_scene_filtered = nullptr; d_scene_score = nullptr; d_filter_info = nullptr;
      scene_filtered_cap = filter_info_cap = 0;
      HIP_RETURN(hipMalloc(&d_scene_filtered, px * sizeof(uint16_t)));
      HIP_RETURN(hipMalloc(&d_scene_score, px * sizeof(uint32_t)));
      HIP_RETURN(hipMalloc(&d_filter_info, (size_t)n_frames * sizeof(lmx::sf::Info)));
      scene_filtered_cap = px; filter_info_cap = (size_t)n_frames;
    }
    HIP_RETURN(hipMemsetAsync(d_filter_info, 0, (size_t)n_frames * sizeof(lmx::sf::Info), on));
    int pe = prof_begin(PK_SCENE_FILTER_SCORE, on);
    lmx::launch_scene_filter_score(on, d_scene, n_frames, W, H, fparams, d_scene_score, d_filter_info);
    prof_end(pe, on);
    HIP_RETURN(hipGetLastError());
    pe = prof_begin(PK_SCENE_FILTER_APPLY, on);
    lmx::launch_scene_filter_apply(on, d_scene, d_scene_score, n_frames, W, H, fparams.stddev_mul, d_scene_filtered, d_filter_info);
    prof_end(pe, on);
    HIP_RETURN(hipGetLastError());
    HIP_RETURN(hipEventRecord(filtered_ready, on));
    return LMX_OK;
  }
  // The scene a pose stage on stream `on` reads, behind the copies of the n_frames W x H frames in d_scene: d_scene itself, or with the filter
  // set their filtered copies, computed there if nobody has.  Without the setting this touches nothing.
  lmx_status pose_scene_on(hipStream_t on, int32_t n_frames, int32_t W, int32_t H, const uint16_t** scene) {
    *scene = d_scene;
    if (!filter_on) return LMX_OK;
    if ((int64_t)W * H > lmx::sf::kMaxFramePixels) {
      lmx::set_error("frames of %d x %d: the scene filter takes at most 2^22 pixels a frame (lmx_depth_templates_set_scene_filter(NULL) turns it off)", W, H);
      return LMX_ERR_INVALID_ARG;
    }
    if (!filtered_ready) HIP_RETURN(hipEventCreateWithFlags(&filtered_ready, hipEventDisableTiming));
    if (scene_filtered_valid) {
      HIP_RETURN(hipStreamWaitEvent(on, filtered_ready, 0));
    } else {
      if (lmx_status st = compute_scene_filtered(on, n_frames, W, H)) return st;
      scene_filtered_valid = true;
    }
    *scene = d_scene_filtered;
    return LMX_OK;
  }
  void free_normal_crops() {
    (void)hipFree(d_ncrops); (void)hipFree(d_ntable);
    d_ncrops = nullptr; d_ntable = nullptr;
    ntable.clear();
  }
  void add(const uint16_t* data, int32_t w, int32_t h, const int32_t rect[4]) {
    table.push_back(lmx::DepthCrop{data, w, h, w > 0 ? lmx::dv::crop_pitch(w) : 0, 0});
    rects.insert(rects.end(), rect, rect + 4);
  }
  ~lmx_depth_templates() {
    if (s) (void)hipStreamSynchronize(s);
    (void)wait_export_reads();
    if (export_read) (void)hipEventDestroy(export_read);
    if (chain_src_ready) (void)hipEventDestroy(chain_src_ready);
    (void)hipFree(chain_rects_refine.dev); (void)hipFree(chain_rects_verify.dev); (void)hipFree(chain_base.dev);
    for (void* p : chunks) (void)hipFree(p);
    (void)hipFree(d_table); (void)hipFree(d_scene); (void)hipFree(d_jobs); (void)hipFree(d_out);
    (void)hipHostFree(h_scene); (void)hipHostFree(h_jobs); (void)hipHostFree(h_out);
    (void)hipFree(d_pjobs); (void)hipFree(d_pout); (void)hipHostFree(h_pjobs); (void)hipHostFree(h_pout);
    (void)hipFree(d_vjobs); (void)hipFree(d_vout); (void)hipHostFree(h_vjobs); (void)hipHostFree(h_vout);
    prof_drain();
    free_normal_crops();
    (void)hipFree(d_angle); (void)hipFree(d_scene_normals); (void)hipFree(d_nout); (void)hipHostFree(h_nout);
    if (normals_ready) (void)hipEventDestroy(normals_ready);
    (void)hipFree(d_scene_filtered); (void)hipFree(d_scene_score); (void)hipFree(d_filter_info);
    if (filtered_ready) (void)hipEventDestroy(filtered_ready);
    if (scene_ready) (void)hipEventDestroy(scene_ready);
    if (scene_src_ready) (void)hipEventDestroy(scene_src_ready);
    if (s) (void)hipStreamDestroy(s);
  }
};

namespace {
struct DeviceBuffer {   // scratch of one call
  void* p = nullptr;
  ~DeviceBuffer() { (void)hipFree(p); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};
size_t crop_bytes(int32_t w, int32_t h) { return (w > 0 && h > 0) ? (size_t)h * (size_t)lmx::dv::crop_pitch(w) * sizeof(uint16_t) : 0; }
}  // namespace

extern "C" lmx_status lmx_depth_templates_from_mesh(int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam,
                                                    const lmx_mesh_view* views, int32_t n_views, lmx_depth_templates** out) {
  return lmx::guarded("lmx_depth_templates_from_mesh", [&]() -> lmx_status {
    using namespace lmx;
    if (!out) { set_error("lmx_depth_templates_from_mesh: null argument"); return LMX_ERR_INVALID_ARG; }
    *out = nullptr;
    mr::Camera dc;
    lmx_status st = mesh_check_args("lmx_depth_templates_from_mesh", triangles, n_triangles, cam, views, n_views, &dc);
    if (st != LMX_OK) return st;
    std::unique_ptr<lmx_depth_templates> t(new lmx_depth_templates);
    t->device = device;
    if (n_views == 0) { *out = t.release(); return LMX_OK; }
    const int bad = mesh_first_invalid_view(triangles, n_triangles, views, n_views);
    if (bad >= 0) { set_error("lmx_depth_templates_from_mesh: view %d puts a vertex at or behind the camera (Z <= 0.01)", bad); return LMX_ERR_INVALID_ARG; }
    if ((st = t->ensure_device()) != LMX_OK) return st;
    static_assert(sizeof(lmx_mesh_view) == 10 * sizeof(double), "lmx_mesh_view is read as 10 doubles");
    const size_t px = (size_t)dc.W * dc.H;
    const int B = std::min<int>(n_views, kCropBatch);
    DeviceBuffer d_tri, d_views, d_work, d_state, d_depth;
    std::vector<int32_t> state((size_t)B * kMeshStateWords);
    hipStream_t s = t->s;
    HIP_RETURN(hipMalloc(&d_tri.p, (size_t)n_triangles * 9 * sizeof(double)));
    HIP_RETURN(hipMalloc(&d_views.p, (size_t)B * 10 * sizeof(double)));
    HIP_RETURN(hipMalloc(&d_work.p, (size_t)B * n_triangles * sizeof(mr::Tri)));
    HIP_RETURN(hipMalloc(&d_state.p, state.size() * 4));
    HIP_RETURN(hipMalloc(&d_depth.p, px * B * sizeof(uint16_t)));
    HIP_RETURN(hipMemcpyAsync(d_tri.p, triangles, (size_t)n_triangles * 9 * sizeof(double), hipMemcpyHostToDevice, s));
    for (int first = 0; first < n_views; first += B) {
      const int n = std::min(B, n_views - first);
      HIP_RETURN(hipMemcpyAsync(d_views.p, views + first, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice, s));
      launch_mesh_raster(s, d_tri.as<double>(), n_triangles, dc, d_views.as<double>(), n, 1, d_work.as<mr::Tri>(), d_state.as<int32_t>(), nullptr,
                         d_depth.as<uint16_t>(), nullptr);
      HIP_RETURN(hipGetLastError());
      HIP_RETURN(hipMemcpyAsync(state.data(), d_state.p, (size_t)n * kMeshStateWords * 4, hipMemcpyDeviceToHost, s));
      HIP_RETURN(hipStreamSynchronize(s));
      CropBatch where;
      std::memset(&where, 0, sizeof(where));
      size_t elems = 0;
      for (int i = 0; i < n; ++i) {
        const int32_t* w = &state[(size_t)i * kMeshStateWords];
        if (w[MS_INVALID]) { set_error("lmx_depth_templates_from_mesh: view %d puts a vertex at or behind the camera (Z <= 0.01)", first + i); return LMX_ERR_INVALID_ARG; }
        const int32_t* b = w + MS_LEVEL;
        where.dst_elem[i] = elems;
        if (b[2] >= 0) elems += crop_bytes(b[2] - b[0] + 1, b[3] - b[1] + 1) / sizeof(uint16_t);
      }
      uint16_t* chunk = nullptr;
      if (elems) {
        HIP_RETURN(hipMalloc(&chunk, elems * sizeof(uint16_t)));
        t->chunks.push_back(chunk);
        t->atlas_bytes += elems * sizeof(uint16_t);
        hipLaunchKernelGGL(k_depth_crop, dim3(dv::kCropCopyGrid, (unsigned)n), dim3(256), 0, s, d_depth.as<uint16_t>(), d_state.as<int32_t>(), dc.W, dc.H, chunk, where);
        HIP_RETURN(hipGetLastError());
      }
      for (int i = 0; i < n; ++i) {
        const int32_t* b = &state[(size_t)i * kMeshStateWords] + MS_LEVEL;
        if (b[2] >= 0) {
          const int32_t r[4] = {b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1};
          t->add(chunk + where.dst_elem[i], r[2], r[3], r);
        } else {
          const int32_t r[4] = {0, 0, 0, 0};
          t->add(nullptr, 0, 0, r);
        }
      }
    }
    HIP_RETURN(hipStreamSynchronize(s));   // the scratch buffers go when this returns
    *out = t.release();
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_depth_templates_from_crops(int32_t device, const uint16_t* const* crops, const int32_t* sizes, int32_t n, lmx_depth_templates** out) {
  return lmx::guarded("lmx_depth_templates_from_crops", [&]() -> lmx_status {
    using namespace lmx;
    if (!out || (n > 0 && (!crops || !sizes))) { set_error("lmx_depth_templates_from_crops: null argument"); return LMX_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n < 0) { set_error("lmx_depth_templates_from_crops: n = %d", n); return LMX_ERR_INVALID_ARG; }
    size_t bytes = 0;
    for (int32_t i = 0; i < n; ++i) {
      const int32_t w = sizes[2 * i], h = sizes[2 * i + 1];
      if (w < 0 || h < 0 || w > dv::kMaxCropSide || h > dv::kMaxCropSide) {
        set_error("lmx_depth_templates_from_crops: crop %d is %d x %d (sides 0 .. %d)", i, w, h, dv::kMaxCropSide);
        return LMX_ERR_INVALID_ARG;
      }
      if (w > 0 && h > 0 && !crops[i]) { set_error("lmx_depth_templates_from_crops: crop %d is null", i); return LMX_ERR_INVALID_ARG; }
      bytes += crop_bytes(w, h);
    }
    std::unique_ptr<lmx_depth_templates> t(new lmx_depth_templates);
    t->device = device;
    uint16_t* chunk = nullptr;
    std::vector<uint16_t> packed;
    if (bytes) {
      if (lmx_status st = t->ensure_device()) return st;
      packed.assign(bytes / sizeof(uint16_t), 0);   // the padding is zeros
      HIP_RETURN(hipMalloc(&chunk, bytes));
      t->chunks.push_back(chunk);
      t->atlas_bytes = bytes;
    }
    size_t at = 0;
    for (int32_t i = 0; i < n; ++i) {
      const int32_t w = sizes[2 * i], h = sizes[2 * i + 1];
      if (w > 0 && h > 0) {
        const int32_t pitch = dv::crop_pitch(w), r[4] = {0, 0, w, h};
        for (int32_t y = 0; y < h; ++y) std::memcpy(&packed[at + (size_t)y * pitch], crops[i] + (size_t)y * w, (size_t)w * sizeof(uint16_t));
        t->add(chunk + at, w, h, r);
        at += (size_t)h * pitch;
      } else {
        const int32_t r[4] = {0, 0, 0, 0};
        t->add(nullptr, 0, 0, r);
      }
    }
    if (bytes) {
      HIP_RETURN(hipMemcpyAsync(chunk, packed.data(), bytes, hipMemcpyHostToDevice, t->s));
      HIP_RETURN(hipStreamSynchronize(t->s));
    }
    *out = t.release();
    return LMX_OK;
  });
}

extern "C" int32_t lmx_depth_templates_count(const lmx_depth_templates* t) { return t ? (int32_t)t->table.size() : 0; }

extern "C" lmx_status lmx_depth_templates_rect(const lmx_depth_templates* t, int32_t id, int32_t rect[4]) {
  if (!t || !rect) { lmx::set_error("lmx_depth_templates_rect: null argument"); return LMX_ERR_INVALID_ARG; }
  if (id < 0 || (size_t)id >= t->table.size()) { lmx::set_error("lmx_depth_templates_rect: id %d outside [0, %zu)", id, t->table.size()); return LMX_ERR_INVALID_ARG; }
  std::memcpy(rect, &t->rects[(size_t)id * 4], 4 * sizeof(int32_t));
  return LMX_OK;
}

extern "C" lmx_status lmx_depth_templates_get(const lmx_depth_templates* ct, int32_t id, uint16_t* out) {
  return lmx::guarded("lmx_depth_templates_get", [&]() -> lmx_status {
    lmx_depth_templates* t = const_cast<lmx_depth_templates*>(ct);   // the stream and the mutex are the object's
    if (!t) { lmx::set_error("lmx_depth_templates_get: null argument"); return LMX_ERR_INVALID_ARG; }
    if (id < 0 || (size_t)id >= t->table.size()) { lmx::set_error("lmx_depth_templates_get: id %d outside [0, %zu)", id, t->table.size()); return LMX_ERR_INVALID_ARG; }
    const lmx::DepthCrop& c = t->table[id];
    if (c.w <= 0 || c.h <= 0) return LMX_OK;
    if (!out) { lmx::set_error("lmx_depth_templates_get: null argument"); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    if (lmx_status st = t->ensure_device()) return st;
    HIP_RETURN(hipMemcpy2DAsync(out, (size_t)c.w * 2, c.data, (size_t)c.pitch * 2, (size_t)c.w * 2, (size_t)c.h, hipMemcpyDeviceToHost, t->s));
    HIP_RETURN(hipStreamSynchronize(t->s));
    return LMX_OK;
  });
}

extern "C" size_t lmx_depth_templates_device_bytes(const lmx_depth_templates* t) {
  if (!t) return 0;
  const size_t depth = t->atlas_bytes + t->table.size() * sizeof(lmx::DepthCrop);
  // with normals: 8 bytes per crop element next to its 2, one address per template
  return t->normals_on ? depth + t->atlas_bytes * (sizeof(lmx::nv::Packed) / sizeof(uint16_t)) + t->table.size() * sizeof(lmx::nv::Packed*) : depth;
}

extern "C" lmx_status lmx_depth_templates_append(lmx_depth_templates* dst, lmx_depth_templates* src) {
  return lmx::guarded("lmx_depth_templates_append", [&]() -> lmx_status {
    if (!dst || !src) { lmx::set_error("lmx_depth_templates_append: null argument"); return LMX_ERR_INVALID_ARG; }
    if (dst == src) { lmx::set_error("lmx_depth_templates_append: an object cannot be appended to itself"); return LMX_ERR_INVALID_ARG; }
    if (dst->device != src->device) {
      lmx::set_error("lmx_depth_templates_append: the objects live on devices %d and %d", dst->device, src->device);
      return LMX_ERR_INVALID_ARG;
    }
    std::mutex* const first = std::less<lmx_depth_templates*>()(dst, src) ? &dst->m : &src->m;
    std::mutex* const second = first == &dst->m ? &src->m : &dst->m;
    std::lock_guard<std::mutex> lk1(*first);
    std::lock_guard<std::mutex> lk2(*second);
    if (src->table.size() + dst->table.size() > 0x7fffffffull) { lmx::set_error("lmx_depth_templates_append: too many templates"); return LMX_ERR_INVALID_ARG; }
    // nothing queued may still read a table or the normals that go
    for (lmx_depth_templates* t : {dst, src})
      if (t->s) {
        HIP_RETURN(hipSetDevice(t->device));
        HIP_RETURN(hipStreamSynchronize(t->s));
        if (lmx_status st = t->wait_export_reads()) return st;
        t->scene_pending = false;
        t->prof_drain();
      }
    dst->table.insert(dst->table.end(), src->table.begin(), src->table.end());
    dst->rects.insert(dst->rects.end(), src->rects.begin(), src->rects.end());
    dst->chunks.insert(dst->chunks.end(), src->chunks.begin(), src->chunks.end());
    dst->atlas_bytes += src->atlas_bytes;
    src->table.clear(); src->rects.clear(); src->chunks.clear(); src->atlas_bytes = 0;
    for (lmx_depth_templates* t : {dst, src}) {
      if (t->d_table) { (void)hipFree(t->d_table); t->d_table = nullptr; }   // uploaded again by ensure_device
      if (t->d_ncrops || t->d_ntable) t->free_normal_crops();                  // recomputed by need_normals
      t->ntable.clear();
      t->ncrops_ready = false;
    }
    dst->scene_frames = 0;                                                     // the scene is forgotten: upload_scene comes before the next scored call
    dst->scene_normals_valid = dst->scene_filtered_valid = false;
    return LMX_OK;
  });
}

extern "C" void lmx_depth_templates_free(lmx_depth_templates* t) {
  if (!t) return;
  if (t->s) (void)hipSetDevice(t->device);
  delete t;
}

namespace {
// 16UC1 host frames of one size, any row stride: what lmx_depth_diff_matches and lmx_depth_templates_upload_scene take
lmx_status check_depth_frames(const char* what, const lmx_image* depth, int32_t n_frames) {
  using namespace lmx;
  const int32_t W = depth[0].cols, H = depth[0].rows;
  for (int32_t f = 0; f < n_frames; ++f) {
    const lmx_image& im = depth[f];
    if (!im.data) { set_error("%s: depth image %d has no data", what, f); return LMX_ERR_INVALID_ARG; }
    if (im.channels != 1 || im.elem_size != 2) { set_error("%s: depth image %d must be one channel of 2 bytes (got %d x %d bytes)", what, f, im.channels, im.elem_size); return LMX_ERR_SHAPE; }
    if (im.rows <= 0 || im.cols <= 0 || im.row_stride_bytes < (size_t)im.cols * 2) { set_error("%s: depth image %d is %d x %d with a row stride of %zu bytes", what, f, im.cols, im.rows, im.row_stride_bytes); return LMX_ERR_SHAPE; }
    if (im.rows != H || im.cols != W) { set_error("%s: depth image %d is %d x %d, image 0 is %d x %d", what, f, im.cols, im.rows, W, H); return LMX_ERR_SHAPE; }
  }
  return LMX_OK;
}

// Stage frame `f` of the caller into slot `slot` of the pinned buffer and queue its copy to the same slot on the device.
lmx_status queue_frame(lmx_depth_templates* t, const lmx_image& im, int32_t slot, int32_t W, int32_t H) {
  const size_t frame_bytes = (size_t)W * H * sizeof(uint16_t);
  uint8_t* h = reinterpret_cast<uint8_t*>(t->h_scene) + frame_bytes * slot;
  lmx::copy_rows(h, im.data, (size_t)W * 2, im.row_stride_bytes, H);
  HIP_RETURN(hipMemcpyAsync(reinterpret_cast<uint8_t*>(t->d_scene) + frame_bytes * slot, h, frame_bytes, hipMemcpyHostToDevice, t->s));
  return LMX_OK;
}

// The device half of a depth check on the host's match list: the first n entries of h_jobs against the W x H frames already in d_scene
// (a job's frame is its slot there): job upload, the walk (depth_launch_walk, the job form), read-back into h_out.  The object's mutex is
// the caller's to hold.  With `normals`: both terms, against the normals of the n_frames frames there (computed first if nobody has), h_nout too.
lmx_status run_jobs(lmx_depth_templates* t, size_t n, int32_t n_frames, int32_t W, int32_t H, bool normals) {
  hipStream_t s = t->s;
  HIP_RETURN(hipMemcpyAsync(t->d_jobs, t->h_jobs, n * sizeof(lmx::DepthJob), hipMemcpyHostToDevice, s));
  lmx::DepthWalk w;
  w.jobs = t->d_jobs; w.n = (uint32_t)n; w.n_frames = n_frames; w.W = W; w.H = H;
  w.d_diffs = t->d_out; w.d_ndiffs = normals ? t->d_nout : nullptr;
  if (lmx_status st = lmx::depth_launch_walk(t, s, w)) return st;
  HIP_RETURN(hipMemcpyAsync(t->h_out, t->d_out, n * sizeof(lmx_depth_diff_t), hipMemcpyDeviceToHost, s));
  if (normals) HIP_RETURN(hipMemcpyAsync(t->h_nout, t->d_nout, n * sizeof(lmx_normal_diff_t), hipMemcpyDeviceToHost, s));
  HIP_RETURN(hipStreamSynchronize(s));
  return LMX_OK;
}

// What lmx_depth_templates_enable_normals needs before any normal-scored call works on the device: normals of every crop.
lmx_status compute_crop_normals(lmx_depth_templates* t) {
  using namespace lmx;
  if (lmx_status st = t->ensure_device()) return st;
  if (lmx_status st = t->ensure_normal_device()) return st;
  HIP_RETURN(hipStreamSynchronize(t->s));
  if (lmx_status st = t->wait_export_reads()) return st;   // an export's walk may still read the normals that go
  t->free_normal_crops();
  t->ncrops_ready = false;
  const size_t n = t->table.size(), elems = t->atlas_bytes / sizeof(uint16_t);
  if (n == 0) { t->ncrops_ready = true; return LMX_OK; }
  if (elems) HIP_RETURN(hipMalloc(&t->d_ncrops, elems * sizeof(nv::Packed)));
  HIP_RETURN(hipMalloc(&t->d_ntable, n * sizeof(nv::Packed*)));
  t->ntable.assign(n, nullptr);
  size_t at = 0;
  for (size_t i = 0; i < n; ++i) {
    const DepthCrop& c = t->table[i];
    if (c.w <= 0 || c.h <= 0) continue;
    t->ntable[i] = t->d_ncrops + at;
    at += (size_t)c.h * (size_t)c.pitch;
  }
  HIP_RETURN(hipMemcpyAsync(t->d_ntable, t->ntable.data(), n * sizeof(nv::Packed*), hipMemcpyHostToDevice, t->s));
  for (size_t first = 0; first < n; first += 32768) {   // blockIdx.y: at most 65535
    const unsigned cnt = (unsigned)std::min<size_t>(32768, n - first);
    hipLaunchKernelGGL(k_normal_map_crops, dim3(nv::kCropMapGrid, cnt), dim3(256), 0, t->s, t->d_table + first, t->d_ntable + first, t->nparams);
    HIP_RETURN(hipGetLastError());
  }
  HIP_RETURN(hipStreamSynchronize(t->s));   // ntable's bytes have left the host
  t->ncrops_ready = true;
  return LMX_OK;
}
// A normal-scored call: refused under the caller's name (`what`, or none) before enable_normals; otherwise, before it touches the device,
// the object's stream, the angle table and the crops' normals.  With `device` false only the refusal: for the two entry points that check
// their other arguments, without a device, before they come back here.
lmx_status need_normals(lmx_depth_templates* t, const char* what, bool device = true) {
  if (!t->normals_on) {
    lmx::set_error("%s%scall lmx_depth_templates_enable_normals first", what ? what : "", what ? ": " : "");
    return LMX_ERR_INVALID_ARG;
  }
  if (!device) return LMX_OK;
  if (lmx_status st = t->ensure_device()) return st;
  if (lmx_status st = t->ensure_normal_device()) return st;
  return t->ncrops_ready ? LMX_OK : compute_crop_normals(t);
}

// The shared end of both match-list paths: matches[sel[k]] as job k against the n_frames W x H frames in d_scene (its frame there is
// sel_slot[k], or `frame` for all of them when sel_slot is null), then out[sel[k]] / nout[sel[k]] (either may be null; nout decides whether
// the normal term is computed).  The caller has zeroed out / nout and made the device ready.
lmx_status diff_selected(lmx_depth_templates* t, const lmx_match_t* matches, const int32_t* sel_slot, int32_t frame, int32_t n_frames, int32_t W, int32_t H,
                         lmx_depth_diff_t* out, lmx_normal_diff_t* nout) {
  const size_t n_sel = t->sel.size();
  if (lmx_status st = t->grow_jobs(n_sel, nout != nullptr)) return st;
  for (size_t k = 0; k < n_sel; ++k) {
    const lmx_match_t& m = matches[t->sel[k]];
    t->h_jobs[k] = lmx::DepthJob{m.x, m.y, m.template_id, sel_slot ? sel_slot[k] : frame};
  }
  if (lmx_status st = run_jobs(t, n_sel, n_frames, W, H, nout != nullptr)) return st;
  for (size_t k = 0; k < n_sel; ++k) {
    if (out) out[t->sel[k]] = t->h_out[k];
    if (nout) nout[t->sel[k]] = t->h_nout[k];
  }
  return LMX_OK;
}
}  // namespace

extern "C" double lmx_depth_value(const lmx_depth_diff_t* diff, double no_value) { return diff ? lmx::dv::value(*diff, no_value) : no_value; }

extern "C" lmx_status lmx_depth_templates_upload_scene(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames) {
  return lmx::guarded("lmx_depth_templates_upload_scene", [&]() -> lmx_status {
    if (!t || !depth) { lmx::set_error("lmx_depth_templates_upload_scene: null argument"); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    return lmx::depth_upload_scene(t, depth, n_frames);
  });
}

// The scene from device memory: pitch-aware device-to-device copies on the object's stream, between an event recorded on the caller's
// stream (the copies read the frames behind everything queued there so far) and a wait of that stream for scene_ready (what is queued
// there afterwards may overwrite or free the frames).  No staging buffer and no host wait; every refusal comes before anything is queued.
extern "C" lmx_status lmx_depth_templates_upload_scene_device(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, void* stream) {
  return lmx::guarded("lmx_depth_templates_upload_scene_device", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_depth_templates_upload_scene_device";
    if (!t || !depth) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    if (n_frames < 1) { set_error("%s: n_frames = %d", what, n_frames); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = check_depth_frames(what, depth, n_frames)) return st;
    if (lmx_status st = t->ensure_device()) return st;
    hipStream_t user = static_cast<hipStream_t>(stream);
    for (int32_t f = 0; f < n_frames; ++f) {
      const lmx_image& im = depth[f];
      if (((uintptr_t)im.data | im.row_stride_bytes) & 1u) { set_error("%s: depth image %d: the address and the row stride must be even", what, f); return LMX_ERR_INVALID_ARG; }
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, im.data) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: depth image %d is not device memory (lmx_depth_templates_upload_scene takes host images)", what, f);
        return LMX_ERR_INVALID_ARG;
      }
      if (attr.type != hipMemoryTypeDevice || attr.device != t->device) {
        set_error("%s: depth image %d is not plain device memory of device %d", what, f, t->device);
        return LMX_ERR_INVALID_ARG;
      }
    }
    if (lmx_status st = check_user_stream(what, user)) return st;
    const int32_t W = depth[0].cols, H = depth[0].rows;
    const size_t frame_bytes = (size_t)W * H * sizeof(uint16_t);
    t->scene_frames = 0;
    t->scene_normals_valid = t->scene_filtered_valid = false;
    if (lmx_status st = t->grow_scene(frame_bytes * (size_t)n_frames)) return st;
    if (!t->scene_src_ready) HIP_RETURN(hipEventCreateWithFlags(&t->scene_src_ready, hipEventDisableTiming));
    HIP_RETURN(hipEventRecord(t->scene_src_ready, user));
    HIP_RETURN(hipStreamWaitEvent(t->s, t->scene_src_ready, 0));
    if (t->export_read_pending) HIP_RETURN(hipStreamWaitEvent(t->s, t->export_read, 0));   // on the device: an export's walk may still read the old scene
    for (int32_t f = 0; f < n_frames; ++f)
      if (hipError_t e = hipMemcpy2DAsync(reinterpret_cast<uint8_t*>(t->d_scene) + frame_bytes * f, (size_t)W * 2, depth[f].data, depth[f].row_stride_bytes, (size_t)W * 2,
                                          (size_t)H, hipMemcpyDeviceToDevice, t->s)) {
        t->drain_after_error();
        set_error("hipMemcpy2DAsync failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
        return LMX_ERR_HIP;
      }
    if (hipError_t e = hipEventRecord(t->scene_ready, t->s)) {
      t->drain_after_error();
      set_error("hipEventRecord failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
      return LMX_ERR_HIP;
    }
    t->scene_frames = n_frames; t->scene_W = W; t->scene_H = H;
    HIP_RETURN(hipStreamWaitEvent(user, t->scene_ready, 0));
    return LMX_OK;
  });
}

namespace lmx {

std::mutex& depth_templates_mutex(lmx_depth_templates* t) { return t->m; }

DepthSceneInfo depth_templates_scene(const lmx_depth_templates* t) {
  return DepthSceneInfo{t->device, (int32_t)t->table.size(), t->scene_frames, t->scene_W, t->scene_H, t->normals_on ? 1 : 0};
}

lmx_status depth_upload_scene(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames) {
  if (n_frames < 1) { set_error("lmx_depth_templates_upload_scene: n_frames = %d", n_frames); return LMX_ERR_INVALID_ARG; }
  if (lmx_status st = check_depth_frames("lmx_depth_templates_upload_scene", depth, n_frames)) return st;
  const int32_t W = depth[0].cols, H = depth[0].rows;
  if (lmx_status st = t->ensure_device()) return st;
  if (lmx_status st = t->wait_scene_copies()) return st;   // the previous scene's copies still read the staging buffer
  if (lmx_status st = t->wait_export_reads()) return st;   // an export's walk may still read the scene these copies overwrite
  t->scene_frames = 0;
  t->scene_normals_valid = t->scene_filtered_valid = false;
  if (lmx_status st = t->grow_scene((size_t)W * H * sizeof(uint16_t) * (size_t)n_frames)) return st;
  for (int32_t f = 0; f < n_frames; ++f)   // each frame on its way while the next is staged
    if (lmx_status st = queue_frame(t, depth[f], f, W, H)) { t->drain_after_error(); return st; }
  if (hipError_t e = hipEventRecord(t->scene_ready, t->s)) {
    t->drain_after_error();
    set_error("hipEventRecord failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    return LMX_ERR_HIP;
  }
  t->scene_pending = true;
  t->scene_frames = n_frames; t->scene_W = W; t->scene_H = H;
  return LMX_OK;   // no host synchronisation: the transfer overlaps whatever the caller queued before
}

lmx_status depth_diff_resident(lmx_depth_templates* t, const lmx_match_t* matches, size_t n, int32_t frame, int32_t class_index, lmx_depth_diff_t* out,
                               lmx_normal_diff_t* nout) {
  if (n == 0) return LMX_OK;
  if (frame < 0 || frame >= t->scene_frames) { set_error("frame %d is not in the uploaded scene (%d frames)", frame, t->scene_frames); return LMX_ERR_INVALID_ARG; }
  if (n > 0x7fffffffull) { set_error("%zu matches in one frame", n); return LMX_ERR_INVALID_ARG; }
  std::memset(out, 0, n * sizeof(lmx_depth_diff_t));
  if (nout) std::memset(nout, 0, n * sizeof(lmx_normal_diff_t));
  const size_t count = t->table.size();
  t->sel.clear();
  for (size_t i = 0; i < n; ++i) {
    const lmx_match_t& m = matches[i];
    if (class_index >= 0 && m.class_index != class_index) continue;
    if (m.template_id < 0 || (size_t)m.template_id >= count) continue;   // zeros, as the record walk gives; the cluster step refuses the id
    t->sel.push_back((uint32_t)i);
  }
  if (t->sel.empty()) return LMX_OK;
  if (nout)
    if (lmx_status st = need_normals(t, nullptr)) return st;
  return diff_selected(t, matches, nullptr, frame, t->scene_frames, t->scene_W, t->scene_H, out, nout);   // on the object's stream, behind the scene's copies
}

// Workgroups of the persistent walk per compute unit.  profiles/export_clusters.txt: the smallest of the grids measured whose time lies
// within the run-to-run spread of the best.
constexpr int kWalkGridPerCU = 4;

namespace {
template <bool NORMALS>
void launch_walk(hipStream_t s, unsigned grid, bool device_count, int src, const WalkArgs& a) {
  const dim3 g(grid), b(256);
  if (device_count) {
    if (src == WALK_RECORDS_CLASSES) hipLaunchKernelGGL((k_walk_records_dev<NORMALS, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_walk_records_dev<NORMALS, false>), g, b, 0, s, a);
    return;
  }
  switch (src) {
    case WALK_JOBS: hipLaunchKernelGGL((k_walk<NORMALS, WALK_JOBS>), g, b, 0, s, a); break;
    case WALK_RECORDS: hipLaunchKernelGGL((k_walk<NORMALS, WALK_RECORDS>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((k_walk<NORMALS, WALK_RECORDS_CLASSES>), g, b, 0, s, a); break;
  }
}
}  // namespace

lmx_status depth_launch_walk(lmx_depth_templates* t, hipStream_t s, const DepthWalk& w) {
  const bool jobs = w.jobs != nullptr, device_count = w.hdr != nullptr, normals = w.d_ndiffs != nullptr;
  const int src = jobs ? WALK_JOBS : (w.d_class_base ? WALK_RECORDS_CLASSES : WALK_RECORDS);
  int32_t n_frames = w.n_frames, W = w.W, H = w.H;
  if (!jobs) {   // records walk against the uploaded scene; the job form's caller has staged frames that are no scene and made the device ready
    if (t->scene_frames < 1) { set_error("no scene uploaded: call lmx_depth_templates_upload_scene first"); return LMX_ERR_INVALID_ARG; }
    if (normals)
      if (lmx_status st = need_normals(t, nullptr)) return st;
    n_frames = t->scene_frames; W = t->scene_W; H = t->scene_H;
  }
  unsigned grid = w.n;
  if (device_count) {
    if (lmx_status st = t->ensure_device()) return st;   // the table, after an append: an export checks nothing else of the object first
    if (!t->export_read) HIP_RETURN(hipEventCreateWithFlags(&t->export_read, hipEventDisableTiming));
    if (w.grid <= 0 && t->walk_grid <= 0) {
      int cus = 0;
      HIP_RETURN(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device));
      t->walk_grid = kWalkGridPerCU * std::max(cus, 1);
    }
    grid = (unsigned)(w.grid > 0 ? w.grid : t->walk_grid);
    // this form alone: nobody waits for it on the host, so the record below must stand behind every earlier such walk too.  A host-count
    // walk ends synchronised, and the collect's stream must not start waiting for exports
    if (t->export_read_pending) HIP_RETURN(hipStreamWaitEvent(s, t->export_read, 0));
  }
  if (!jobs) HIP_RETURN(hipStreamWaitEvent(s, t->scene_ready, 0));   // the job form runs on the stream that carries the frames' copies
  if (!device_count && w.n == 0) return LMX_OK;   // a grid of 0 is no launch; the device-count form launches always: nobody here knows the count
  if (normals)   // the scene's normals first, on this stream, if this is the scene's first normal-scored call
    if (lmx_status st = t->scene_normals_on(s, nullptr, n_frames, W, H)) return st;
  const WalkArgs a{t->d_table, t->d_ntable, w.hdr, w.recs, w.cap, (int32_t)t->table.size(), w.class_index, w.d_class_base, w.n_classes, t->d_scene,
                   t->d_scene_normals, n_frames, W, H, t->d_angle, w.d_diffs, w.d_ndiffs, w.jobs};
  using PK = lmx_depth_templates;
  // the depth-only job walk has never had a bracket: the labels are public (DepthTemplates.KERNELS) and there is none for it
  const int label = device_count ? PK::PK_WALK_RECORDS_DEV : jobs ? (normals ? PK::PK_VERIFY_DIFF : -1) : (normals ? PK::PK_VERIFY_DIFF_RECORDS : PK::PK_DEPTH_DIFF_RECORDS);
  const int pe = label >= 0 ? t->prof_begin(label, s) : -1;
  if (normals) launch_walk<true>(s, grid, device_count, src, a);
  else launch_walk<false>(s, grid, device_count, src, a);
  t->prof_end(pe, s);
  HIP_RETURN(hipGetLastError());
  if (device_count) {   // what changes the crops, the scene or the normals waits for this
    HIP_RETURN(hipEventRecord(t->export_read, s));
    t->export_read_pending = true;
  }
  return LMX_OK;
}

lmx_status depth_diff_resident_classes(lmx_depth_templates* t, const lmx_match_t* matches, size_t n, int32_t frame, const int32_t* class_base, int32_t n_classes,
                                       lmx_depth_diff_t* out, lmx_normal_diff_t* nout) {
  // the matches with their crop's index in the joined object for a template id; what record_class_job leaves out becomes id -1: zeros
  std::vector<lmx_match_t> joined(matches, matches + n);
  for (lmx_match_t& m : joined) {
    int32_t id = -1;
    if (m.class_index >= 0 && m.class_index < n_classes && m.template_id >= 0 && m.template_id < class_base[m.class_index + 1] - class_base[m.class_index])
      id = class_base[m.class_index] + m.template_id;
    m.template_id = id;
  }
  return depth_diff_resident(t, joined.data(), n, frame, -1, out, nout);
}

}  // namespace lmx

namespace {
// The body of lmx_depth_diff_matches (nout null) and lmx_normal_diff_matches (nout: the normal sums; out may then be null).
lmx_status diff_matches_impl(const char* what, lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                             const size_t* offsets, int32_t class_index, lmx_depth_diff_t* out, lmx_normal_diff_t* nout, bool normals) {
    using namespace lmx;
    if (!t) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    if (normals)
      if (lmx_status st = need_normals(t, what, false)) return st;
    if (n_frames < 0) { set_error("%s: n_frames = %d", what, n_frames); return LMX_ERR_INVALID_ARG; }
    if (n_frames == 0) return LMX_OK;
    if (!depth || !offsets) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    if (offsets[0] != 0) { set_error("%s: offsets[0] = %zu (expected 0)", what, offsets[0]); return LMX_ERR_INVALID_ARG; }
    for (int32_t f = 0; f < n_frames; ++f)
      if (offsets[f + 1] < offsets[f]) { set_error("%s: offsets[%d] = %zu is below offsets[%d] = %zu", what, f + 1, offsets[f + 1], f, offsets[f]); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = check_depth_frames(what, depth, n_frames)) return st;
    const int32_t W = depth[0].cols, H = depth[0].rows;
    const size_t n_matches = offsets[n_frames];
    if (n_matches == 0) return LMX_OK;
    if (!matches || (normals ? !nout : !out)) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    if (n_matches > 0x7fffffffull) { set_error("%s: %zu matches in one call", what, n_matches); return LMX_ERR_INVALID_ARG; }   // sel holds uint32, the grid is n_sel wide
    std::lock_guard<std::mutex> lk(t->m);
    const size_t count = t->table.size();
    t->sel.clear();
    t->sel_slot.clear();
    t->slot.assign((size_t)n_frames, -1);
    int32_t n_slots = 0;
    for (int32_t f = 0; f < n_frames; ++f)
      for (size_t i = offsets[f]; i < offsets[f + 1]; ++i) {
        const lmx_match_t& m = matches[i];
        if (class_index >= 0 && m.class_index != class_index) continue;
        if (m.template_id < 0 || (size_t)m.template_id >= count) { set_error("%s: match %zu: template_id %d outside [0, %zu)", what, i, m.template_id, count); return LMX_ERR_INVALID_ARG; }
        if (t->slot[f] < 0) t->slot[f] = n_slots++;
        t->sel.push_back((uint32_t)i);
        t->sel_slot.push_back(t->slot[f]);
      }
    if (out) std::memset(out, 0, n_matches * sizeof(lmx_depth_diff_t));
    if (normals) std::memset(nout, 0, n_matches * sizeof(lmx_normal_diff_t));
    if (t->sel.empty()) return LMX_OK;
    if (lmx_status st = normals ? need_normals(t, what) : t->ensure_device()) return st;
    const size_t frame_bytes = (size_t)W * H * sizeof(uint16_t);
    // the frames that have matches take the place of an uploaded scene: staged row by row into pinned memory, each on its way while the
    // next is staged
    if (lmx_status st = t->wait_scene_copies()) return st;
    if (lmx_status st = t->wait_export_reads()) return st;   // an export's walk may still read the scene the staged frames replace
    t->scene_frames = 0;
    t->scene_normals_valid = t->scene_filtered_valid = false;
    if (lmx_status st = t->grow_scene(frame_bytes * n_slots)) return st;
    for (int32_t f = 0; f < n_frames; ++f)
      if (t->slot[f] >= 0)
        if (lmx_status st = queue_frame(t, depth[f], t->slot[f], W, H)) { t->drain_after_error(); return st; }
    const lmx_status st = diff_selected(t, matches, t->sel_slot.data(), 0, n_slots, W, H, out, normals ? nout : nullptr);
    if (st != LMX_OK) t->drain_after_error();
    t->scene_normals_valid = t->scene_filtered_valid = false;   // they belong to staged frames that are no scene
    return st;
}
}  // namespace

extern "C" lmx_status lmx_depth_diff_matches(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                                             const size_t* offsets, int32_t class_index, lmx_depth_diff_t* out) {
  return lmx::guarded("lmx_depth_diff_matches", [&]() -> lmx_status {
    return diff_matches_impl("lmx_depth_diff_matches", t, depth, n_frames, matches, offsets, class_index, out, nullptr, false);
  });
}

extern "C" lmx_status lmx_normal_diff_matches(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                                              const size_t* offsets, int32_t class_index, lmx_depth_diff_t* ddiffs, lmx_normal_diff_t* out) {
  return lmx::guarded("lmx_normal_diff_matches", [&]() -> lmx_status {
    return diff_matches_impl("lmx_normal_diff_matches", t, depth, n_frames, matches, offsets, class_index, ddiffs, out, true);
  });
}

extern "C" double lmx_match_value(const lmx_depth_diff_t* ddiff, const lmx_normal_diff_t* ndiff, double no_value) {
  return ddiff && ndiff ? lmx::nv::value(*ddiff, *ndiff, no_value) : no_value;
}

extern "C" lmx_status lmx_normal_angle_table(uint32_t* out) {
  if (!out) { lmx::set_error("lmx_normal_angle_table: null argument"); return LMX_ERR_INVALID_ARG; }
  lmx::nv::build_angle_table(out);
  return LMX_OK;
}

extern "C" lmx_status lmx_depth_templates_enable_normals(lmx_depth_templates* t, const lmx_normal_params* params) {
  return lmx::guarded("lmx_depth_templates_enable_normals", [&]() -> lmx_status {
    using namespace lmx;
    if (!t || !params) { set_error("lmx_depth_templates_enable_normals: null argument"); return LMX_ERR_INVALID_ARG; }
    const float fx = (float)params->fx, fy = (float)params->fy;
    if (!(fx > 0.0f) || !(fy > 0.0f) || !(fx <= 1.0e6f) || !(fy <= 1.0e6f)) {   // 1e6 x |ddx| < 1e9 squared stays a finite float
      set_error("lmx_depth_templates_enable_normals: fx = %g, fy = %g (focal lengths in pixels: above 0, at most 1e6)", params->fx, params->fy);
      return LMX_ERR_INVALID_ARG;
    }
    if (params->difference_threshold < 1 || params->distance_threshold < 1) {
      set_error("lmx_depth_templates_enable_normals: difference_threshold = %d, distance_threshold = %d (both >= 1)", params->difference_threshold,
                params->distance_threshold);
      return LMX_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(t->m);
    const nv::Params np = {fx, fy, params->difference_threshold, params->distance_threshold};
    if (t->normals_on && t->ncrops_ready && std::memcmp(&np, &t->nparams, sizeof(np)) == 0) return LMX_OK;
    if (lmx_status st = t->wait_export_reads()) return st;   // the scene's normals are computed again: an export's walk may still read them
    t->nparams = np;
    t->normals_on = true;
    t->ncrops_ready = false;
    t->scene_normals_valid = t->scene_filtered_valid = false;
    if (t->atlas_bytes == 0) return LMX_OK;   // no pixel to take a normal of: nothing needs the device yet
    if (lmx_status st = compute_crop_normals(t)) { t->normals_on = false; return st; }
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_depth_templates_get_normals(const lmx_depth_templates* ct, int32_t id, int16_t* out) {
  return lmx::guarded("lmx_depth_templates_get_normals", [&]() -> lmx_status {
    lmx_depth_templates* t = const_cast<lmx_depth_templates*>(ct);
    if (!t) { lmx::set_error("lmx_depth_templates_get_normals: null argument"); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = need_normals(t, "lmx_depth_templates_get_normals", false)) return st;
    if (id < 0 || (size_t)id >= t->table.size()) { lmx::set_error("lmx_depth_templates_get_normals: id %d outside [0, %zu)", id, t->table.size()); return LMX_ERR_INVALID_ARG; }
    const lmx::DepthCrop& c = t->table[id];
    if (c.w <= 0 || c.h <= 0) return LMX_OK;
    if (!out) { lmx::set_error("lmx_depth_templates_get_normals: null argument"); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    if (lmx_status st = need_normals(t, "lmx_depth_templates_get_normals")) return st;
    HIP_RETURN(hipMemcpy2DAsync(out, (size_t)c.w * 8, t->ntable[id], (size_t)c.pitch * 8, (size_t)c.w * 8, (size_t)c.h, hipMemcpyDeviceToHost, t->s));
    HIP_RETURN(hipStreamSynchronize(t->s));
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_depth_templates_set_profiling(lmx_depth_templates* t, int32_t on) {
  if (!t) { lmx::set_error("lmx_depth_templates_set_profiling: null argument"); return LMX_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(t->m);
  t->prof_drain();
  if (on && !t->profiling)
    for (int k = 0; k < lmx_depth_templates::PK_COUNT; ++k) { t->prof_ms[k] = 0.0; t->prof_launches[k] = 0; }
  t->profiling = on != 0;
  return LMX_OK;
}

extern "C" lmx_status lmx_depth_templates_kernel_time(lmx_depth_templates* t, int32_t kernel, double* total_ms, int64_t* launches) {
  if (!t || !total_ms || !launches) { lmx::set_error("lmx_depth_templates_kernel_time: null argument"); return LMX_ERR_INVALID_ARG; }
  if (kernel < 0 || kernel >= lmx_depth_templates::PK_COUNT) { lmx::set_error("lmx_depth_templates_kernel_time: kernel %d outside [0, %d)", kernel, (int)lmx_depth_templates::PK_COUNT); return LMX_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(t->m);
  t->prof_drain();   // waits for the launches still in flight
  *total_ms = t->prof_ms[kernel];
  *launches = t->prof_launches[kernel];
  return LMX_OK;
}

extern "C" lmx_status lmx_debug_scene_normals(lmx_depth_templates* t, int32_t frame, int16_t* out) {
  return lmx::guarded("lmx_debug_scene_normals", [&]() -> lmx_status {
    if (!t || !out) { lmx::set_error("lmx_debug_scene_normals: null argument"); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    if (lmx_status st = need_normals(t, "lmx_debug_scene_normals", false)) return st;
    if (t->scene_frames < 1) { lmx::set_error("lmx_debug_scene_normals: no scene uploaded: call lmx_depth_templates_upload_scene first"); return LMX_ERR_INVALID_ARG; }
    if (frame < 0 || frame >= t->scene_frames) { lmx::set_error("lmx_debug_scene_normals: frame %d is not in the uploaded scene (%d frames)", frame, t->scene_frames); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = need_normals(t, "lmx_debug_scene_normals")) return st;
    if (lmx_status st = t->scene_normals_on(t->s, nullptr, t->scene_frames, t->scene_W, t->scene_H)) return st;
    const size_t px = (size_t)t->scene_W * t->scene_H;
    HIP_RETURN(hipMemcpyAsync(out, t->d_scene_normals + px * frame, px * sizeof(lmx::nv::Packed), hipMemcpyDeviceToHost, t->s));
    HIP_RETURN(hipStreamSynchronize(t->s));
    return LMX_OK;
  });
}

// ---- the scene filter: the host half (the kernels: lmx_scene_filter.hip) ------------------------------------------------------------------------------
static_assert(sizeof(lmx_scene_filter_info) == sizeof(lmx::sf::Info) && sizeof(lmx_scene_filter_info) == 56 && sizeof(lmx_scene_filter_params) == 56, "layouts of the scene filter");

extern "C" lmx_status lmx_scene_filter_defaults(lmx_scene_filter_params* out) {
  if (!out) { lmx::set_error("lmx_scene_filter_defaults: null argument"); return LMX_ERR_INVALID_ARG; }
  *out = lmx_scene_filter_params{(uint32_t)sizeof(lmx_scene_filter_params), 3, 15, 0, 1.0, 0.0, 0.0, 0.0, 0.0};
  return LMX_OK;
}

extern "C" lmx_status lmx_depth_templates_set_scene_filter(lmx_depth_templates* t, const lmx_scene_filter_params* p) {
  return lmx::guarded("lmx_depth_templates_set_scene_filter", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_depth_templates_set_scene_filter";
    if (!t) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    sf::Params P = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0, 0};
    if (p) {
      if (p->struct_size != sizeof(lmx_scene_filter_params)) { set_error("%s: params->struct_size = %u (expected %zu)", what, p->struct_size, sizeof(lmx_scene_filter_params)); return LMX_ERR_INVALID_ARG; }
      if (p->reserved != 0) { set_error("%s: reserved = %d (must be 0)", what, p->reserved); return LMX_ERR_INVALID_ARG; }
      P = sf::Params{{p->fx, p->fy, p->cx, p->cy}, p->stddev_mul, p->radius, p->k};
      if (const char* why = sf::check_params(P)) { set_error("%s: %s (radius %d, k %d, stddev_mul %g, camera %g %g %g %g)", what, why, p->radius, p->k, p->stddev_mul, p->fx, p->fy, p->cx, p->cy); return LMX_ERR_INVALID_ARG; }
    }
    std::lock_guard<std::mutex> lk(t->m);
    t->fparams = P;   // queued work reads the copy made under the old setting; the next call makes its own, behind it on the object's stream
    t->filter_on = p != nullptr;
    t->scene_filtered_valid = false;
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_debug_scene_filtered(lmx_depth_templates* t, int32_t frame, uint16_t* out, lmx_scene_filter_info* out_info) {
  return lmx::guarded("lmx_debug_scene_filtered", [&]() -> lmx_status {
    const char* what = "lmx_debug_scene_filtered";
    if (!t || !out) { lmx::set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    if (!t->filter_on) { lmx::set_error("%s: call lmx_depth_templates_set_scene_filter first", what); return LMX_ERR_INVALID_ARG; }
    if (t->scene_frames < 1) { lmx::set_error("%s: no scene uploaded: call lmx_depth_templates_upload_scene first", what); return LMX_ERR_INVALID_ARG; }
    if (frame < 0 || frame >= t->scene_frames) { lmx::set_error("%s: frame %d is not in the uploaded scene (%d frames)", what, frame, t->scene_frames); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = t->ensure_device()) return st;
    HIP_RETURN(hipStreamWaitEvent(t->s, t->scene_ready, 0));
    const uint16_t* scene = nullptr;
    if (lmx_status st = t->pose_scene_on(t->s, t->scene_frames, t->scene_W, t->scene_H, &scene)) return st;
    const size_t px = (size_t)t->scene_W * t->scene_H;
    HIP_RETURN(hipMemcpyAsync(out, scene + px * frame, px * sizeof(uint16_t), hipMemcpyDeviceToHost, t->s));
    if (out_info) HIP_RETURN(hipMemcpyAsync(out_info, t->d_filter_info + frame, sizeof(lmx_scene_filter_info), hipMemcpyDeviceToHost, t->s));
    HIP_RETURN(hipStreamSynchronize(t->s));
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_debug_depth_walk_grid(lmx_depth_templates* t, int32_t workgroups) {
  if (!t || workgroups < 0 || workgroups > 65536) { lmx::set_error("lmx_debug_depth_walk_grid: templates must not be null, workgroups 0 .. 65536"); return LMX_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(t->m);
  t->walk_grid = workgroups;
  return LMX_OK;
}

// The walk of lmx_ctx_export_clusters_on on a slot the caller builds: header {n_candidates, header_count}, the records behind it, a grid the
// caller chooses.  diffs / ndiffs go to the device as they are and come back as the kernel left them.
extern "C" lmx_status lmx_debug_depth_walk_records(lmx_depth_templates* t, const lmx_raw_match_t* records, size_t n_records, uint32_t header_count,
                                                   uint32_t n_candidates, uint32_t cap, int32_t grid_workgroups, int32_t class_index, const int32_t* class_base,
                                                   int32_t n_classes, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs) {
  return lmx::guarded("lmx_debug_depth_walk_records", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_debug_depth_walk_records";
    if (!t || !diffs || (n_records && !records)) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    if (grid_workgroups < 1 || grid_workgroups > 65536) { set_error("%s: grid_workgroups %d outside 1 .. 65536", what, grid_workgroups); return LMX_ERR_INVALID_ARG; }
    if (n_records > ((size_t)1 << 24)) { set_error("%s: at most 2^24 records", what); return LMX_ERR_INVALID_ARG; }
    // the kernel walks header_count records unless the header says that a list overflowed: they must all be the caller's
    if (!xpack::list_overflowed(n_candidates, header_count, cap) && header_count > n_records) {
      set_error("%s: the header counts %u records, %zu were passed", what, header_count, n_records);
      return LMX_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(t->m);
    if (class_base) {
      if (n_classes < 1 || n_classes > F2_CLASSES || class_base[0] != 0) { set_error("%s: class_base: n_classes 1..%d, class_base[0] = 0", what, F2_CLASSES); return LMX_ERR_INVALID_ARG; }
      for (int32_t k = 0; k < n_classes; ++k)
        if (class_base[k + 1] < class_base[k]) { set_error("%s: class_base must not decrease", what); return LMX_ERR_INVALID_ARG; }
      if ((size_t)class_base[n_classes] != t->table.size()) { set_error("%s: class_base ends at %d but the object holds %zu depth templates", what, class_base[n_classes], t->table.size()); return LMX_ERR_INVALID_ARG; }
    }
    if (ndiffs)
      if (lmx_status st = need_normals(t, what, false)) return st;
    if (t->scene_frames < 1) { set_error("%s: no scene uploaded: call lmx_depth_templates_upload_scene first", what); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = t->ensure_device()) return st;
    const size_t R = std::max<size_t>(n_records, 1);
    DeviceBuffer d_hdr, d_recs, d_base, d_diffs, d_ndiffs;
    uint32_t hdr[16] = {0};
    hdr[0] = n_candidates; hdr[1] = header_count;
    hipStream_t s = t->s;
    HIP_RETURN(hipMalloc(&d_hdr.p, sizeof(hdr)));
    HIP_RETURN(hipMalloc(&d_recs.p, R * sizeof(lmx_raw_match_t)));
    HIP_RETURN(hipMalloc(&d_diffs.p, R * sizeof(lmx_depth_diff_t)));
    HIP_RETURN(hipMemcpyAsync(d_hdr.p, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
    if (n_records) {
      HIP_RETURN(hipMemcpyAsync(d_recs.p, records, n_records * sizeof(lmx_raw_match_t), hipMemcpyHostToDevice, s));
      HIP_RETURN(hipMemcpyAsync(d_diffs.p, diffs, n_records * sizeof(lmx_depth_diff_t), hipMemcpyHostToDevice, s));
    }
    if (ndiffs) {
      HIP_RETURN(hipMalloc(&d_ndiffs.p, R * sizeof(lmx_normal_diff_t)));
      if (n_records) HIP_RETURN(hipMemcpyAsync(d_ndiffs.p, ndiffs, n_records * sizeof(lmx_normal_diff_t), hipMemcpyHostToDevice, s));
    }
    if (class_base) {
      HIP_RETURN(hipMalloc(&d_base.p, ((size_t)n_classes + 1) * sizeof(int32_t)));
      HIP_RETURN(hipMemcpyAsync(d_base.p, class_base, ((size_t)n_classes + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    DepthWalk w;
    w.recs = d_recs.as<lmx_raw_match_t>(); w.hdr = d_hdr.as<uint32_t>(); w.cap = cap; w.grid = grid_workgroups;
    w.class_index = class_index; w.d_class_base = d_base.as<int32_t>(); w.n_classes = class_base ? n_classes : 0;
    w.d_diffs = d_diffs.as<lmx_depth_diff_t>(); w.d_ndiffs = d_ndiffs.as<lmx_normal_diff_t>();
    lmx_status st = depth_launch_walk(t, s, w);
    if (st == LMX_OK && n_records) {
      HIP_RETURN(hipMemcpyAsync(diffs, d_diffs.p, n_records * sizeof(lmx_depth_diff_t), hipMemcpyDeviceToHost, s));
      if (ndiffs) HIP_RETURN(hipMemcpyAsync(ndiffs, d_ndiffs.p, n_records * sizeof(lmx_normal_diff_t), hipMemcpyDeviceToHost, s));
    }
    HIP_RETURN(hipStreamSynchronize(s));   // the scratch buffers go when this returns
    t->export_read_pending = false;
    return st;
  });
}

// ---- pose refinement: the host half -------------------------------------------------------------------------------------------------------------------
namespace {
// The parameters as the header takes them, or why they are refused: before any device work.
lmx_status pose_params(const char* what, const lmx_pose_refine_params* p, lmx::pr::Params* out) {
  using namespace lmx;
  if (!p) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  if (p->struct_size != sizeof(lmx_pose_refine_params)) {
    set_error("%s: params->struct_size = %u (expected %zu)", what, p->struct_size, sizeof(lmx_pose_refine_params));
    return LMX_ERR_INVALID_ARG;
  }
  const pr::Params P = {{p->model_fx, p->model_fy, p->model_cx, p->model_cy}, {p->scene_fx, p->scene_fy, p->scene_cx, p->scene_cy},
                        p->max_dist_mm, p->eps_rot_rad, p->eps_trans_mm, p->max_iterations, p->min_pairs, p->search_radius, 0};
  if (const char* why = pr::check_params(P)) { set_error("%s: %s", what, why); return LMX_ERR_INVALID_ARG; }
  *out = P;
  return LMX_OK;
}

// What lmx_pose_refine_matches and lmx_pose_verify_matches share, everything around the launch: the argument checks, the selection of the
// matches of the class (t->sel, t->sel_slot), the zeroed records, the staging of the frames that have matches or the wait for the
// resident scene, the draining after an error.
struct PoseCall {
  const char* what;
  lmx_depth_templates* t;
  const lmx_image* depth;
  int32_t n_frames;
  const lmx_match_t* matches;
  const size_t* offsets;
  int32_t class_index;
  const int32_t* rects;      // the caller's, or null for the object's own
  void* out;
  size_t record_bytes;
  bool input_missing;        // another per-match array of the call is null
  int64_t max_pixels;        // W * H may not exceed it (0: no such limit)
};
// select(i, m): 1 the match is computed, 0 it keeps its zeroed record, -1 it is refused (the error is set).  selected(): after the records
// were zeroed, before any device work.  launch(W, H, n_slots, count, rects): queues the work on t->s behind the scene and waits for it.
lmx_status pose_call(const PoseCall& a, const std::function<int(size_t, const lmx_match_t&)>& select, const std::function<void()>& selected,
                     const std::function<lmx_status(int32_t, int32_t, int32_t, size_t, const int32_t*)>& launch) {
  using namespace lmx;
  const char* what = a.what;
  lmx_depth_templates* t = a.t;
  const lmx_image* depth = a.depth;
  const int32_t n_frames = a.n_frames;
  const size_t* offsets = a.offsets;
  if (n_frames < 0) { set_error("%s: n_frames = %d", what, n_frames); return LMX_ERR_INVALID_ARG; }
  if (n_frames == 0) return LMX_OK;
  if (!offsets) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  if (offsets[0] != 0) { set_error("%s: offsets[0] = %zu (expected 0)", what, offsets[0]); return LMX_ERR_INVALID_ARG; }
  for (int32_t f = 0; f < n_frames; ++f)
    if (offsets[f + 1] < offsets[f]) { set_error("%s: offsets[%d] = %zu is below offsets[%d] = %zu", what, f + 1, offsets[f + 1], f, offsets[f]); return LMX_ERR_INVALID_ARG; }
  if (depth)
    if (lmx_status st = check_depth_frames(what, depth, n_frames)) return st;
  std::lock_guard<std::mutex> lk(t->m);
  if (!depth && t->scene_frames < 1) { set_error("%s: depth is null and no scene is uploaded: call lmx_depth_templates_upload_scene first", what); return LMX_ERR_INVALID_ARG; }
  if (!depth && t->scene_frames != n_frames) { set_error("%s: depth is null and the uploaded scene holds %d frames, not %d", what, t->scene_frames, n_frames); return LMX_ERR_INVALID_ARG; }
  const int32_t W = depth ? depth[0].cols : t->scene_W, H = depth ? depth[0].rows : t->scene_H;
  if (W >= pr::kMaxCoord / 2 || H >= pr::kMaxCoord / 2) { set_error("%s: frames of %d x %d (sides below %d)", what, W, H, (int)(pr::kMaxCoord / 2)); return LMX_ERR_INVALID_ARG; }
  if (a.max_pixels > 0 && (int64_t)W * H > a.max_pixels) { set_error("%s: frames of %d x %d (at most %lld pixels)", what, W, H, (long long)a.max_pixels); return LMX_ERR_INVALID_ARG; }
  if (t->filter_on && (int64_t)W * H > sf::kMaxFramePixels) { set_error("%s: frames of %d x %d (at most 2^22 pixels while the scene filter is set)", what, W, H); return LMX_ERR_INVALID_ARG; }
  const size_t n_matches = offsets[n_frames];
  if (n_matches == 0) return LMX_OK;
  if (!a.matches || !a.out || a.input_missing) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  if (n_matches > 0x7fffffffull) { set_error("%s: %zu matches in one call", what, n_matches); return LMX_ERR_INVALID_ARG; }
  const size_t count = t->table.size();
  const int32_t* rects = a.rects ? a.rects : t->rects.data();
  t->sel.clear();
  t->sel_slot.clear();
  t->slot.assign((size_t)n_frames, -1);
  int32_t n_slots = 0;
  for (int32_t f = 0; f < n_frames; ++f)
    for (size_t i = offsets[f]; i < offsets[f + 1]; ++i) {
      const lmx_match_t& m = a.matches[i];
      if (a.class_index >= 0 && m.class_index != a.class_index) continue;
      if (m.template_id < 0 || (size_t)m.template_id >= count) { set_error("%s: match %zu: template_id %d outside [0, %zu)", what, i, m.template_id, count); return LMX_ERR_INVALID_ARG; }
      const int32_t* r = rects + (size_t)m.template_id * 4;
      const int32_t lim = (int32_t)(pr::kMaxCoord / 2);   // a corner within +-2^17 and sides <= 2^14 keep |u|, |v| below 2^18
      if (r[0] < -lim || r[0] > lim || r[1] < -lim || r[1] > lim) { set_error("%s: match %zu: the rect of template %d starts at (%d, %d) (within +-%d)", what, i, m.template_id, r[0], r[1], lim); return LMX_ERR_INVALID_ARG; }
      const int take = select ? select(i, m) : 1;
      if (take < 0) return LMX_ERR_INVALID_ARG;
      if (take == 0) continue;
      if (t->slot[f] < 0) t->slot[f] = depth ? n_slots++ : f;
      t->sel.push_back((uint32_t)i);
      t->sel_slot.push_back(t->slot[f]);
    }
  if (!depth) n_slots = t->scene_frames;
  std::memset(a.out, 0, n_matches * a.record_bytes);
  if (selected) selected();
  if (t->sel.empty()) return LMX_OK;
  if (lmx_status st = t->ensure_device()) return st;
  hipStream_t s = t->s;
  if (depth) {
    // the frames that have matches take the place of an uploaded scene, as in lmx_depth_diff_matches
    const size_t frame_bytes = (size_t)W * H * sizeof(uint16_t);
    if (lmx_status st = t->wait_scene_copies()) return st;
    if (lmx_status st = t->wait_export_reads()) return st;   // an export's walk may still read the scene the staged frames replace
    t->scene_frames = 0;
    t->scene_normals_valid = t->scene_filtered_valid = false;
    if (lmx_status st = t->grow_scene(frame_bytes * n_slots)) return st;
    for (int32_t f = 0; f < n_frames; ++f)
      if (t->slot[f] >= 0)
        if (lmx_status st = queue_frame(t, depth[f], t->slot[f], W, H)) { t->drain_after_error(); return st; }
  } else {
    HIP_RETURN(hipStreamWaitEvent(s, t->scene_ready, 0));   // the resident scene: behind its copies, whichever stream queued them
  }
  const lmx_status st = launch(W, H, n_slots, count, rects);
  if (st != LMX_OK) t->drain_after_error();
  if (depth) t->scene_filtered_valid = false;   // it belongs to staged frames that are no scene
  return st;
}

// The body of lmx_pose_refine_matches and of its test hooks (dbg: the sums of job 0's passes, [max_iterations + 1][17], under a schedule
// [sum of its max_iterations + 1][17]; dbg_plane, only next to dbg: the same rows of the 29 plane sums).  With a point_shift >= 0 in force
// (lmx_depth_templates_set_refine_plane) the PLANE kernel runs, behind the normals of the frames in d_scene -- resident or staged.
lmx_status pose_refine_impl(const char* what, lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches, const size_t* offsets,
                            int32_t class_index, const lmx_pose_refine_params* params, lmx_pose_refine_t* out, int64_t* dbg, int64_t* dbg_plane = nullptr) {
  using namespace lmx;
  if (!t) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  pr::Params P;
  if (lmx_status st = pose_params(what, params, &P)) return st;
  const PoseCall call = {what, t, depth, n_frames, matches, offsets, class_index, params->rects, out, sizeof(lmx_pose_refine_t), false, 0};
  pr::Schedule S = pr::single_stage(P);
  pr::PlaneShifts K = pr::kNoPlane;
  bool plane = false;
  return pose_call(
      call, nullptr,
      [&]() {   // t->m is held from here on
        S = t->schedule_for(P);
        K = t->plane;
        plane = t->plane_for(S);
        if (dbg) std::memset(dbg, 0, (size_t)pr::schedule_passes(S) * pr::kSums * sizeof(int64_t));
        if (dbg_plane) std::memset(dbg_plane, 0, (size_t)pr::schedule_passes(S) * pr::kPlaneSums * sizeof(int64_t));
      },
      [&](int32_t W, int32_t H, int32_t n_slots, size_t count, const int32_t* rects) -> lmx_status {
        hipStream_t s = t->s;
        const size_t n = t->sel.size();
        if (lmx_status g = lmx_depth_templates::grow_pair(t->d_pjobs, t->h_pjobs, t->pjobs_cap, n)) return g;
        if (lmx_status g = lmx_depth_templates::grow_pair(t->d_pout, t->h_pout, t->pout_cap, n)) return g;
        for (size_t k = 0; k < n; ++k) {
          const lmx_match_t& m = matches[t->sel[k]];
          const int32_t* r = rects + (size_t)m.template_id * 4;
          t->h_pjobs[k] = PoseJob{m.x, m.y, m.template_id, t->sel_slot[k], r[0], r[1], 0, 0};
        }
        DeviceBuffer d_dbg;
        const size_t rows = (size_t)pr::schedule_passes(S), row = plane ? pr::kAllSums : pr::kSums;   // the PLANE kernel's rows hold all 46
        const size_t dbg_bytes = rows * row * sizeof(int64_t);
        std::vector<int64_t> h_dbg;
        const uint16_t* scene = nullptr;   // the frames in d_scene, or with the scene filter set their filtered copies
        if (lmx_status g = t->pose_scene_on(s, n_slots, W, H, &scene)) return g;
        if (plane)
          if (lmx_status g = t->plane_normals_on(s, n_slots, W, H)) return g;
        if (dbg) {
          HIP_RETURN(hipMalloc(&d_dbg.p, dbg_bytes));
          HIP_RETURN(hipMemsetAsync(d_dbg.p, 0, dbg_bytes, s));
        }
        HIP_RETURN(hipMemcpyAsync(t->d_pjobs, t->h_pjobs, n * sizeof(PoseJob), hipMemcpyHostToDevice, s));
        const int pe = t->prof_begin(lmx_depth_templates::PK_POSE_REFINE, s);
        if (plane)
          hipLaunchKernelGGL(k_pose_refine<true>, dim3((unsigned)n), dim3(256), 0, s, t->d_table, (int32_t)count, t->d_pjobs, scene, n_slots, W, H, P, S, t->d_pout,
                             d_dbg.as<long long>(), t->d_scene_normals, K);
        else
          hipLaunchKernelGGL(k_pose_refine<false>, dim3((unsigned)n), dim3(256), 0, s, t->d_table, (int32_t)count, t->d_pjobs, scene, n_slots, W, H, P, S, t->d_pout,
                             d_dbg.as<long long>(), nullptr, K);
        t->prof_end(pe, s);
        HIP_RETURN(hipGetLastError());
        HIP_RETURN(hipMemcpyAsync(t->h_pout, t->d_pout, n * sizeof(lmx_pose_refine_t), hipMemcpyDeviceToHost, s));
        if (dbg) {
          if (plane) h_dbg.resize(rows * row);
          HIP_RETURN(hipMemcpyAsync(plane ? h_dbg.data() : dbg, d_dbg.p, dbg_bytes, hipMemcpyDeviceToHost, s));
        }
        HIP_RETURN(hipStreamSynchronize(s));   // the results are here, the scratch buffer may go
        if (depth) t->scene_normals_valid = false;   // they belong to staged frames that are no scene
        for (size_t k = 0; k < n; ++k) out[t->sel[k]] = t->h_pout[k];
        for (size_t r = 0; r < rows && dbg && plane; ++r) {
          std::memcpy(dbg + r * pr::kSums, &h_dbg[r * row], pr::kSums * sizeof(int64_t));
          if (dbg_plane) std::memcpy(dbg_plane + r * pr::kPlaneSums, &h_dbg[r * row + pr::kSums], pr::kPlaneSums * sizeof(int64_t));
        }
        return LMX_OK;
      });
}

// The parameters of lmx_pose_verify_matches as the header takes them, or why they are refused: before any device work.
lmx_status verify_params(const char* what, const lmx_pose_verify_params* p, lmx::pv::Params* out) {
  using namespace lmx;
  if (!p) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  if (p->struct_size != sizeof(lmx_pose_verify_params)) {
    set_error("%s: params->struct_size = %u (expected %zu)", what, p->struct_size, sizeof(lmx_pose_verify_params));
    return LMX_ERR_INVALID_ARG;
  }
  const pv::Params P = {{p->model_fx, p->model_fy, p->model_cx, p->model_cy}, {p->scene_fx, p->scene_fy, p->scene_cx, p->scene_cy}, p->voxel_mm, p->roi_margin, 0};
  if (const char* why = pv::check_params(P)) { set_error("%s: %s", what, why); return LMX_ERR_INVALID_ARG; }
  *out = P;
  return LMX_OK;
}
}  // namespace

extern "C" lmx_status lmx_pose_refine_matches(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches, const size_t* offsets,
                                              int32_t class_index, const lmx_pose_refine_params* params, lmx_pose_refine_t* out) {
  return lmx::guarded("lmx_pose_refine_matches", [&]() -> lmx_status {
    return pose_refine_impl("lmx_pose_refine_matches", t, depth, n_frames, matches, offsets, class_index, params, out, nullptr);
  });
}

extern "C" lmx_status lmx_debug_pose_refine_sums(lmx_depth_templates* t, const lmx_image* depth, const lmx_match_t* match, const lmx_pose_refine_params* params,
                                                 lmx_pose_refine_t* out, int64_t* sums) {
  return lmx::guarded("lmx_debug_pose_refine_sums", [&]() -> lmx_status {
    if (!depth || !match || !out || !sums) { lmx::set_error("lmx_debug_pose_refine_sums: null argument"); return LMX_ERR_INVALID_ARG; }
    const size_t offsets[2] = {0, 1};
    return pose_refine_impl("lmx_debug_pose_refine_sums", t, depth, 1, match, offsets, -1, params, out, sums);
  });
}

extern "C" lmx_status lmx_debug_pose_refine_plane_sums(lmx_depth_templates* t, const lmx_image* depth, const lmx_match_t* match, const lmx_pose_refine_params* params,
                                                       lmx_pose_refine_t* out, int64_t* sums, int64_t* plane_sums) {
  return lmx::guarded("lmx_debug_pose_refine_plane_sums", [&]() -> lmx_status {
    if (!depth || !match || !out || !sums || !plane_sums) { lmx::set_error("lmx_debug_pose_refine_plane_sums: null argument"); return LMX_ERR_INVALID_ARG; }
    const size_t offsets[2] = {0, 1};
    return pose_refine_impl("lmx_debug_pose_refine_plane_sums", t, depth, 1, match, offsets, -1, params, out, sums, plane_sums);
  });
}

extern "C" lmx_status lmx_depth_templates_set_refine_plane(lmx_depth_templates* t, const int32_t* point_shift, int32_t n_stages) {
  return lmx::guarded("lmx_depth_templates_set_refine_plane", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_depth_templates_set_refine_plane";
    if (!t) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    if (const char* why = pr::check_plane(point_shift, n_stages)) { set_error("%s: %s (n_stages = %d)", what, why, n_stages); return LMX_ERR_INVALID_ARG; }
    pr::PlaneShifts K = pr::kNoPlane;
    if (point_shift)
      for (int32_t k = 0; k < n_stages; ++k) K.shift[k] = point_shift[k];
    std::lock_guard<std::mutex> lk(t->m);
    if (pr::any_plane(K, pr::kMaxStages) && !t->normals_on) {
      set_error("%s: a point_shift >= 0 reads the scene's normals: call lmx_depth_templates_enable_normals first", what);
      return LMX_ERR_INVALID_ARG;
    }
    t->plane = K;   // queued work took its shifts by value: nothing to wait for
    t->plane_stages = point_shift ? n_stages : 0;
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_depth_templates_get_refine_plane(const lmx_depth_templates* t, int32_t out[LMX_POSE_MAX_STAGES], int32_t* n_stages) {
  return lmx::guarded("lmx_depth_templates_get_refine_plane", [&]() -> lmx_status {
    if (!t || !out || !n_stages) { lmx::set_error("lmx_depth_templates_get_refine_plane: null argument"); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(const_cast<lmx_depth_templates*>(t)->m);
    *n_stages = t->plane_stages;
    for (int32_t k = 0; k < LMX_POSE_MAX_STAGES; ++k) out[k] = t->plane.shift[k];
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_depth_templates_set_refine_schedule(lmx_depth_templates* t, const lmx_pose_refine_stage* stages, int32_t n_stages) {
  return lmx::guarded("lmx_depth_templates_set_refine_schedule", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_depth_templates_set_refine_schedule";
    if (!t) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    if (n_stages < 0 || n_stages > LMX_POSE_MAX_STAGES) { set_error("%s: n_stages = %d (0 .. %d)", what, n_stages, (int)LMX_POSE_MAX_STAGES); return LMX_ERR_INVALID_ARG; }
    if (n_stages > 0 && !stages) { set_error("%s: stages is null with n_stages = %d", what, n_stages); return LMX_ERR_INVALID_ARG; }
    pr::Schedule S = {n_stages, 0, {}};
    for (int32_t k = 0; k < n_stages; ++k) {
      const lmx_pose_refine_stage& g = stages[k];
      if (g.reserved != 0) { set_error("%s: stage %d: reserved = %d (must be 0)", what, k, g.reserved); return LMX_ERR_INVALID_ARG; }
      S.stage[k] = pr::Stage{g.max_dist_mm, g.eps_rot_rad, g.eps_trans_mm, g.max_iterations, g.search_radius, g.stride, 0};
    }
    if (n_stages > 0)
      if (const char* why = pr::check_schedule(S)) { set_error("%s: %s", what, why); return LMX_ERR_INVALID_ARG; }   // a NaN fails its range
    std::lock_guard<std::mutex> lk(t->m);
    t->schedule = S;   // queued work took its schedule by value: nothing to wait for
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_depth_templates_get_refine_schedule(const lmx_depth_templates* t, lmx_pose_refine_stage out[LMX_POSE_MAX_STAGES], int32_t* n_stages) {
  return lmx::guarded("lmx_depth_templates_get_refine_schedule", [&]() -> lmx_status {
    if (!t || !out || !n_stages) { lmx::set_error("lmx_depth_templates_get_refine_schedule: null argument"); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(const_cast<lmx_depth_templates*>(t)->m);
    *n_stages = t->schedule.n_stages;
    for (int32_t k = 0; k < LMX_POSE_MAX_STAGES; ++k) {
      const lmx::pr::Stage z = {0.0, 0.0, 0.0, 0, 0, 0, 0};
      const lmx::pr::Stage& g = k < t->schedule.n_stages ? t->schedule.stage[k] : z;
      out[k] = lmx_pose_refine_stage{g.max_dist_mm, g.eps_rot_rad, g.eps_trans_mm, g.max_iterations, g.search_radius, g.stride, 0};
    }
    return LMX_OK;
  });
}

extern "C" lmx_status lmx_pose_compose(const lmx_mesh_view* view, const lmx_pose_refine_t* refined, double R_obj[9], double t_obj_m[3]) {
  if (!view || !refined || !R_obj || !t_obj_m) { lmx::set_error("lmx_pose_compose: null argument"); return LMX_ERR_INVALID_ARG; }
  const double* R = refined->R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R_obj[3 * i + j] = (R[3 * i] * view->R[j] + R[3 * i + 1] * view->R[3 + j]) + R[3 * i + 2] * view->R[6 + j];
  const double z = 1000.0 * view->distance;
  for (int i = 0; i < 3; ++i) t_obj_m[i] = (R[3 * i + 2] * z + refined->t_mm[i]) / 1000.0;
  return LMX_OK;
}

// ---- pose verification: the host half -----------------------------------------------------------------------------------------------------------------
extern "C" lmx_status lmx_pose_verify_matches(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches, const size_t* offsets,
                                              int32_t class_index, const lmx_pose_refine_t* poses, const lmx_pose_verify_params* params, lmx_pose_verify_t* out) {
  return lmx::guarded("lmx_pose_verify_matches", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_pose_verify_matches";
    if (!t) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    pv::Params P;
    if (lmx_status st = verify_params(what, params, &P)) return st;
    const PoseCall call = {what, t, depth, n_frames, matches, offsets, class_index, params->rects, out, sizeof(lmx_pose_verify_t), poses == nullptr, INT32_MAX};
    return pose_call(
        call,
        [&](size_t i, const lmx_match_t&) -> int {
          const lmx_pose_refine_t& p = poses[i];
          if (p.status == LMX_POSE_NONE) return 0;   // nothing was refined: a zeroed record
          if (const char* why = pv::check_pose(p.R, p.t_mm)) { set_error("%s: match %zu: %s", what, i, why); return -1; }
          return 1;
        },
        nullptr,
        [&](int32_t W, int32_t H, int32_t n_slots, size_t count, const int32_t* rects) -> lmx_status {
          hipStream_t s = t->s;
          const size_t n = t->sel.size();
          if (lmx_status g = lmx_depth_templates::grow_pair(t->d_vjobs, t->h_vjobs, t->vjobs_cap, n)) return g;
          if (lmx_status g = lmx_depth_templates::grow_pair(t->d_vout, t->h_vout, t->vout_cap, n)) return g;
          for (size_t k = 0; k < n; ++k) {
            const lmx_match_t& m = matches[t->sel[k]];
            const lmx_pose_refine_t& p = poses[t->sel[k]];
            const int32_t* r = rects + (size_t)m.template_id * 4;
            VerifyJob& j = t->h_vjobs[k];
            j.template_id = m.template_id; j.frame = t->sel_slot[k]; j.rect_x = r[0]; j.rect_y = r[1];
            std::memcpy(j.R, p.R, sizeof(j.R));
            std::memcpy(j.t_mm, p.t_mm, sizeof(j.t_mm));
          }
          const uint16_t* scene = nullptr;
          if (lmx_status g = t->pose_scene_on(s, n_slots, W, H, &scene)) return g;
          HIP_RETURN(hipMemcpyAsync(t->d_vjobs, t->h_vjobs, n * sizeof(VerifyJob), hipMemcpyHostToDevice, s));
          const int pe = t->prof_begin(lmx_depth_templates::PK_POSE_VERIFY, s);
          hipLaunchKernelGGL(k_pose_verify, dim3((unsigned)n), dim3(256), 0, s, t->d_table, (int32_t)count, t->d_vjobs, scene, n_slots, W, H, P, t->d_vout);
          t->prof_end(pe, s);
          HIP_RETURN(hipGetLastError());
          HIP_RETURN(hipMemcpyAsync(t->h_vout, t->d_vout, n * sizeof(lmx_pose_verify_t), hipMemcpyDeviceToHost, s));
          HIP_RETURN(hipStreamSynchronize(s));
          for (size_t k = 0; k < n; ++k) out[t->sel[k]] = t->h_vout[k];
          return LMX_OK;
        });
  });
}

extern "C" lmx_status lmx_pose_verify_keep(const lmx_pose_verify_t* records, size_t count, double thresh, uint8_t* keep) {
  if (count == 0) return LMX_OK;
  if (!records || !keep) { lmx::set_error("lmx_pose_verify_keep: null argument"); return LMX_ERR_INVALID_ARG; }
  for (size_t i = 0; i < count; ++i) {
    lmx::pv::Record r;
    std::memcpy(&r, &records[i], sizeof(r));
    keep[i] = lmx::pv::keep(r, thresh) ? 1 : 0;
  }
  return LMX_OK;
}

// ---- both stages on exported clusters: the host half --------------------------------------------------------------------------------------------------
namespace {
// `src` (n entries) in device memory at d.dev: uploaded on first use and when it differs from what the previous call left there.  The
// previous chain's kernels may still read the old entries: the upload waits for them (they run on t->s).
lmx_status chain_sync_ints(lmx_depth_templates* t, lmx_depth_templates::DevInts& d, const int32_t* src, size_t n) {
  if (d.dev && d.host.size() == n && std::equal(d.host.begin(), d.host.end(), src)) return LMX_OK;
  HIP_RETURN(hipStreamSynchronize(t->s));
  if (n > d.cap || !d.dev) {
    (void)hipFree(d.dev);
    d.dev = nullptr; d.cap = 0; d.host.clear();
    const size_t want = std::max<size_t>(n, 1);
    HIP_RETURN(hipMalloc(&d.dev, want * sizeof(int32_t)));
    d.cap = want;
  }
  d.host.clear();
  if (n) HIP_RETURN(hipMemcpy(d.dev, src, n * sizeof(int32_t), hipMemcpyHostToDevice));
  d.host.assign(src, src + n);
  return LMX_OK;
}

// One array of a chain call: plain device memory of the object's device, aligned to its element.
lmx_status check_chain_memory(const char* what, const lmx_depth_templates* t, const char* name, const void* p, size_t align) {
  using namespace lmx;
  if ((uintptr_t)p & (align - 1)) { set_error("%s: %s must be aligned to %zu bytes", what, name, align); return LMX_ERR_INVALID_ARG; }
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {   // memory the runtime has never seen
    (void)hipGetLastError();
    set_error("%s: %s is not device memory", what, name);
    return LMX_ERR_INVALID_ARG;
  }
  if (attr.type != hipMemoryTypeDevice || attr.device != t->device) {
    set_error("%s: %s is %s; the arrays are plain device memory of device %d", what, name,
              attr.type == hipMemoryTypeDevice ? "memory of another device" : "pageable, pinned, managed or other host memory", t->device);
    return LMX_ERR_INVALID_ARG;
  }
  return LMX_OK;
}

// What the checks read of the fields lmx_pose_chain_desc and lmx_rough_chain_desc share.  outputs: the call's own second output stands in
// for `leaders` (the rough chain's member_group).
struct ChainFields {
  const lmx_pose_refine_params* refine;
  const lmx_pose_verify_params* verify;
  bool lists, outputs;   // none of header, frame_info, matches, clusters, members / of chain_header, leaders, poses, checks, keep is null
  size_t cap_clusters;
  int32_t n_frames;
  double keep_thresh;
};
template <typename Desc>
ChainFields chain_fields(const Desc* d, const void* leaders) {
  return {d->refine, d->verify, d->header && d->frame_info && d->matches && d->clusters && d->members, d->chain_header && leaders && d->poses && d->checks && d->keep,
          d->cap_clusters, d->n_frames, d->keep_thresh};
}
template <typename Desc>
lmx::pc::Lists chain_lists(const Desc& d) {
  using namespace lmx;
  return pc::Lists{d.header, d.frame_info, d.n_frames, reinterpret_cast<const pc::Match*>(d.matches), reinterpret_cast<const pc::Cluster*>(d.clusters), d.members,
                   (uint64_t)d.cap_matches, (uint64_t)d.cap_clusters, (uint64_t)d.cap_members};
}

// What both chain calls refuse of the shared fields, whatever memory the arrays live in; t->m is held.
lmx_status chain_check_fields(const char* what, lmx_depth_templates* t, const ChainFields& d, lmx::pr::Params* PR, lmx::pv::Params* PV) {
  using namespace lmx;
  if (lmx_status st = pose_params(what, d.refine, PR)) return st;
  if (lmx_status st = verify_params(what, d.verify, PV)) return st;
  if (!d.lists) { set_error("%s: header, frame_info, matches, clusters and members must not be null", what); return LMX_ERR_INVALID_ARG; }
  if (!d.outputs) { set_error("%s: chain_header, leaders, poses, checks and keep must not be null", what); return LMX_ERR_INVALID_ARG; }
  if (d.cap_clusters < 1 || d.cap_clusters > pc::kMaxClusters) { set_error("%s: cap_clusters = %zu (1 .. 2^20)", what, d.cap_clusters); return LMX_ERR_INVALID_ARG; }
  if (d.n_frames < 1) { set_error("%s: n_frames = %d", what, d.n_frames); return LMX_ERR_INVALID_ARG; }
  if (d.keep_thresh != d.keep_thresh) { set_error("%s: keep_thresh is not a number", what); return LMX_ERR_INVALID_ARG; }
  if (t->scene_frames < 1) { set_error("%s: no scene is uploaded: call lmx_depth_templates_upload_scene first", what); return LMX_ERR_INVALID_ARG; }
  if (t->scene_frames != d.n_frames) { set_error("%s: the uploaded scene holds %d frames, not %d", what, t->scene_frames, d.n_frames); return LMX_ERR_INVALID_ARG; }
  const int32_t W = t->scene_W, H = t->scene_H;
  if (W >= pr::kMaxCoord / 2 || H >= pr::kMaxCoord / 2) { set_error("%s: frames of %d x %d (sides below %d)", what, W, H, (int)(pr::kMaxCoord / 2)); return LMX_ERR_INVALID_ARG; }
  if ((int64_t)W * H > (int64_t)INT32_MAX) { set_error("%s: frames of %d x %d (at most %d pixels)", what, W, H, INT32_MAX); return LMX_ERR_INVALID_ARG; }
  if (t->filter_on && (int64_t)W * H > sf::kMaxFramePixels) { set_error("%s: frames of %d x %d (at most 2^22 pixels while the scene filter is set)", what, W, H); return LMX_ERR_INVALID_ARG; }
  return LMX_OK;
}

// Everything lmx_pose_chain_on refuses that does not depend on where the arrays live; t->m is held.
lmx_status chain_check(const char* what, lmx_depth_templates* t, const lmx_pose_chain_desc* d, lmx::pr::Params* PR, lmx::pv::Params* PV) {
  using namespace lmx;
  if (d->struct_size != sizeof(lmx_pose_chain_desc)) { set_error("%s: struct_size %u, not %zu", what, d->struct_size, sizeof(lmx_pose_chain_desc)); return LMX_ERR_INVALID_ARG; }
  if (lmx_status st = chain_check_fields(what, t, chain_fields(d, d->leaders), PR, PV)) return st;
  if (d->class_base) {
    if (d->n_classes < 1 || d->n_classes > F2_CLASSES || d->class_base[0] != 0) { set_error("%s: class_base: n_classes 1..%d, class_base[0] = 0", what, F2_CLASSES); return LMX_ERR_INVALID_ARG; }
    for (int32_t k = 0; k < d->n_classes; ++k)
      if (d->class_base[k + 1] < d->class_base[k]) { set_error("%s: class_base must not decrease", what); return LMX_ERR_INVALID_ARG; }
    if ((size_t)d->class_base[d->n_classes] != t->table.size()) { set_error("%s: class_base ends at %d but the object holds %zu depth templates", what, d->class_base[d->n_classes], t->table.size()); return LMX_ERR_INVALID_ARG; }
  }
  return LMX_OK;
}

// The front of a chain call's work on t->s: behind what the caller's stream holds (the export's end, and whatever still uses the
// outputs), behind every earlier walk of the export and behind the scene's upload.  user: the caller's stream, with_user false: a test
// hook, which orders nothing but t->s itself.
lmx_status chain_begin(lmx_depth_templates* t, hipStream_t user, bool with_user) {
  if (!t->export_read) HIP_RETURN(hipEventCreateWithFlags(&t->export_read, hipEventDisableTiming));
  if (!t->chain_src_ready) HIP_RETURN(hipEventCreateWithFlags(&t->chain_src_ready, hipEventDisableTiming));
  if (with_user) {
    HIP_RETURN(hipEventRecord(t->chain_src_ready, user));
    HIP_RETURN(hipStreamWaitEvent(t->s, t->chain_src_ready, 0));
  }
  if (t->export_read_pending) HIP_RETURN(hipStreamWaitEvent(t->s, t->export_read, 0));   // chain_end's record then stands behind every earlier walk too
  HIP_RETURN(hipStreamWaitEvent(t->s, t->scene_ready, 0));
  return LMX_OK;
}

// Its end: the record the next export's writes wait for, and the caller's stream behind it.
lmx_status chain_end(lmx_depth_templates* t, hipStream_t user, bool with_user) {
  HIP_RETURN(hipEventRecord(t->export_read, t->s));
  t->export_read_pending = true;
  if (with_user) HIP_RETURN(hipStreamWaitEvent(user, t->export_read, 0));
  return LMX_OK;
}

// Queues the call (every array of `d` in device memory, chain_check passed, t->m held): the tables, chain_begin, the three launches,
// chain_end.
lmx_status chain_queue(lmx_depth_templates* t, const lmx_pose_chain_desc& d, const lmx::pr::Params& PR, const lmx::pv::Params& PV, hipStream_t user, bool with_user) {
  using namespace lmx;
  if (lmx_status st = t->ensure_device()) return st;
  const size_t count = t->table.size();
  const int32_t* rr = d.refine->rects ? d.refine->rects : t->rects.data();
  const int32_t* rv = d.verify->rects ? d.verify->rects : t->rects.data();
  if (lmx_status st = chain_sync_ints(t, t->chain_rects_refine, rr, count * 4)) return st;
  const bool same_rects = rv == rr || std::equal(rr, rr + count * 4, rv);
  if (!same_rects)
    if (lmx_status st = chain_sync_ints(t, t->chain_rects_verify, rv, count * 4)) return st;
  if (d.class_base)
    if (lmx_status st = chain_sync_ints(t, t->chain_base, d.class_base, (size_t)d.n_classes + 1)) return st;
  if (lmx_status st = chain_begin(t, user, with_user)) return st;
  hipStream_t s = t->s;
  ChainArgs a;
  a.L = chain_lists(d);
  a.T =pc::Table{(int32_t)count, t->chain_rects_refine.dev, d.class_base ? -1 : d.class_index, d.class_base ? t->chain_base.dev : nullptr, d.class_base ? d.n_classes : 0};
  a.crops = t->d_table; a.W = t->scene_W; a.H = t->scene_H;
  if (lmx_status st = t->pose_scene_on(s, t->scene_frames, t->scene_W, t->scene_H, &a.scene)) return st;   // an event wait or two launches, nothing on the host
  a.chain_header = d.chain_header; a.leaders = d.leaders; a.poses = d.poses; a.checks = d.checks; a.keep = d.keep; a.keep_thresh = d.keep_thresh;
  const dim3 grid((unsigned)d.cap_clusters), block(256);
  HIP_RETURN(hipMemsetAsync(d.chain_header, 0, pc::C_WORDS * sizeof(uint32_t), s));
  int pe = -1;
  const pr::Schedule S = t->schedule_for(PR);
  if (t->plane_for(S)) {   // the scene's normals first, on this stream: an event wait or one launch, nothing on the host
    if (lmx_status st = t->plane_normals_on(s, t->scene_frames, t->scene_W, t->scene_H)) return st;
    pe = t->prof_begin(lmx_depth_templates::PK_POSE_REFINE_CLUSTERS, s);
    hipLaunchKernelGGL(k_pose_refine_clusters<true>, grid, block, 0, s, a, PR, S, t->d_scene_normals, t->plane);
  } else {
    pe = t->prof_begin(lmx_depth_templates::PK_POSE_REFINE_CLUSTERS, s);
    hipLaunchKernelGGL(k_pose_refine_clusters<false>, grid, block, 0, s, a, PR, S, nullptr, t->plane);
  }
  t->prof_end(pe, s);
  HIP_RETURN(hipGetLastError());
  if (!same_rects) a.T.rects = t->chain_rects_verify.dev;
  pe = t->prof_begin(lmx_depth_templates::PK_POSE_VERIFY_CLUSTERS, s);
  hipLaunchKernelGGL(k_pose_verify_clusters, grid, block, 0, s, a, PV);
  t->prof_end(pe, s);
  HIP_RETURN(hipGetLastError());
  return chain_end(t, user, with_user);
}

// The arrays of a test hook's call, which lie in host memory: {host address, bytes, uploaded only or read back as well}.  upload:
// each in a device buffer of its own, filled on s; at(i): that buffer, for the desc the hook hands on; finish: the outputs back (where
// the call was queued) and the stream drained -- the buffers go with this object.
struct HookArray { const void* host; size_t bytes; bool is_output; };
template <int N>
struct HookArrays {
  const HookArray* arr = nullptr;
  DeviceBuffer dev[N];
  lmx_status upload(const HookArray (&a)[N], hipStream_t s) {
    arr = a;
    for (int k = 0; k < N; ++k) {
      HIP_RETURN(hipMalloc(&dev[k].p, std::max<size_t>(a[k].bytes, 16)));
      if (a[k].bytes) HIP_RETURN(hipMemcpyAsync(dev[k].p, a[k].host, a[k].bytes, hipMemcpyHostToDevice, s));
    }
    return LMX_OK;
  }
  template <typename T> T* at(int k) const { return dev[k].template as<T>(); }
  lmx_status finish(hipStream_t s, bool queued) {
    for (int k = 0; k < N && queued; ++k)
      if (arr[k].is_output && arr[k].bytes) HIP_RETURN(hipMemcpyAsync(const_cast<void*>(arr[k].host), dev[k].p, arr[k].bytes, hipMemcpyDeviceToHost, s));
    HIP_RETURN(hipStreamSynchronize(s));
    return LMX_OK;
  }
};
}  // namespace

extern "C" lmx_status lmx_pose_chain_on(lmx_depth_templates* t, const lmx_pose_chain_desc* d, void* stream) {
  return lmx::guarded("lmx_pose_chain_on", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_pose_chain_on";
    if (!t || !d) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    pr::Params PR;
    pv::Params PV;
    if (lmx_status st = chain_check(what, t, d, &PR, &PV)) return st;
    if (lmx_status st = t->ensure_device()) return st;
    hipStream_t user = static_cast<hipStream_t>(stream);
    if (lmx_status st = check_user_stream(what, user)) return st;
    const struct { const char* name; const void* p; size_t align; } arrays[] = {
        {"header", d->header, 4}, {"frame_info", d->frame_info, 4}, {"matches", d->matches, 4}, {"clusters", d->clusters, 8}, {"members", d->members, 4},
        {"chain_header", d->chain_header, 4}, {"leaders", d->leaders, 4}, {"poses", d->poses, 8}, {"checks", d->checks, 8}, {"keep", d->keep, 1}};
    for (const auto& arr : arrays)
      if (lmx_status st = check_chain_memory(what, t, arr.name, arr.p, arr.align)) return st;
    const lmx_status st = chain_queue(t, *d, PR, PV, user, true);
    if (st != LMX_OK) t->drain_after_error();
    return st;
  });
}

extern "C" lmx_status lmx_debug_pose_chain(lmx_depth_templates* t, const lmx_pose_chain_desc* d) {
  return lmx::guarded("lmx_debug_pose_chain", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_debug_pose_chain";
    if (!t || !d) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    pr::Params PR;
    pv::Params PV;
    if (lmx_status st = chain_check(what, t, d, &PR, &PV)) return st;
    if (d->cap_matches > ((size_t)1 << 24) || d->cap_members > ((size_t)1 << 24)) { set_error("%s: at most 2^24 matches and members", what); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = t->ensure_device()) return st;
    hipStream_t s = t->s;
    const size_t C = d->cap_clusters;
    // five inputs, five outputs (chain_header is zeroed by the call)
    const HookArray arr[10] = {{d->header, xpack::H_WORDS * sizeof(uint32_t), false}, {d->frame_info, (size_t)d->n_frames * xpack::I_WORDS * sizeof(int32_t), false},
                               {d->matches, d->cap_matches * sizeof(lmx_match_t), false}, {d->clusters, C * sizeof(lmx_cluster_t), false},
                               {d->members, d->cap_members * sizeof(int32_t), false}, {d->chain_header, pc::C_WORDS * sizeof(uint32_t), true},
                               {d->leaders, C * sizeof(int32_t), true}, {d->poses, C * sizeof(lmx_pose_refine_t), true}, {d->checks, C * sizeof(lmx_pose_verify_t), true},
                               {d->keep, C, true}};
    HookArrays<10> h;
    if (lmx_status st = h.upload(arr, s)) return st;
    lmx_pose_chain_desc dd = *d;
    dd.header = h.at<uint32_t>(0); dd.frame_info = h.at<int32_t>(1); dd.matches = h.at<lmx_match_t>(2); dd.clusters = h.at<lmx_cluster_t>(3);
    dd.members = h.at<int32_t>(4); dd.chain_header = h.at<uint32_t>(5); dd.leaders = h.at<int32_t>(6); dd.poses = h.at<lmx_pose_refine_t>(7);
    dd.checks = h.at<lmx_pose_verify_t>(8); dd.keep = h.at<uint8_t>(9);
    const lmx_status st = chain_queue(t, dd, PR, PV, nullptr, false);
    if (lmx_status e = h.finish(s, st == LMX_OK)) return e;
    t->export_read_pending = false;
    return st;
  });
}

// ---- the rough pose stage in front of both stages: the host half (the stage: lmx_rough.hip) ----------------------------------------------------------
namespace {
// lmx_pose_chain_on's checks on the fields the two descs share, then the stage's own; t->m and model->m are held.
lmx_status rough_check(const char* what, lmx_depth_templates* t, lmx_rough_model* model, const lmx_rough_chain_desc* d, lmx::pr::Params* PR, lmx::pv::Params* PV) {
  using namespace lmx;
  if (d->struct_size != sizeof(lmx_rough_chain_desc)) { set_error("%s: struct_size %u, not %zu", what, d->struct_size, sizeof(lmx_rough_chain_desc)); return LMX_ERR_INVALID_ARG; }
  if (!d->rough || !d->member_group) { set_error("%s: rough and member_group must not be null", what); return LMX_ERR_INVALID_ARG; }
  if (lmx_status st = chain_check_fields(what, t, chain_fields(d, d->member_group), PR, PV)) return st;
  if (d->refine->rects || d->verify->rects) { set_error("%s: rects must be NULL: the rects are the rendered ones", what); return LMX_ERR_INVALID_ARG; }
  if (d->trace_min != d->trace_min) { set_error("%s: trace_min is not a number", what); return LMX_ERR_INVALID_ARG; }
  if (model->device != t->device) { set_error("%s: the model lives on device %d, the depth templates on device %d", what, model->device, t->device); return LMX_ERR_INVALID_ARG; }
  if (d->cap_clusters > (size_t)model->cap_slots) { set_error("%s: cap_clusters = %zu exceeds the model's cap_slots = %d", what, d->cap_clusters, model->cap_slots); return LMX_ERR_INVALID_ARG; }
  const mr::Camera& c = model->cam;
  const bool same_refine = d->refine->model_fx == c.fx && d->refine->model_fy == c.fy && d->refine->model_cx == c.cx && d->refine->model_cy == c.cy;
  const bool same_verify = d->verify->model_fx == c.fx && d->verify->model_fy == c.fy && d->verify->model_cx == c.cx && d->verify->model_cy == c.cy;
  if (!same_refine || !same_verify) {
    set_error("%s: the model camera of the parameters is not the model's (%g, %g, %g, %g)", what, c.fx, c.fy, c.cx, c.cy);
    return LMX_ERR_INVALID_ARG;
  }
  return LMX_OK;
}

// As chain_queue: chain_begin, the stage, the two pose kernels, chain_end; and the model's own record, in front of and behind its kernels.
lmx_status rough_queue(lmx_depth_templates* t, lmx_rough_model* model, const lmx_rough_chain_desc& d, const lmx::pr::Params& PR, const lmx::pv::Params& PV, hipStream_t user,
                       bool with_user) {
  using namespace lmx;
  if (lmx_status st = t->ensure_device()) return st;
  if (lmx_status st = chain_begin(t, user, with_user)) return st;
  hipStream_t s = t->s;
  if (model->done_pending) HIP_RETURN(hipStreamWaitEvent(s, model->done, 0));   // the model's arena serves one call at a time
  rp::StageArgs a;
  a.L = chain_lists(d);
  a.class_index = d.class_index; a.trace_min = d.trace_min; a.chain_header = d.chain_header;
  a.rough = reinterpret_cast<rp::Record*>(d.rough); a.member_group = d.member_group;
  HIP_RETURN(hipMemsetAsync(d.chain_header, 0, pc::C_WORDS * sizeof(uint32_t), s));
  launch_rough_stage(s, model, a);
  HIP_RETURN(hipGetLastError());
  const uint16_t* scene = nullptr;
  if (lmx_status st = t->pose_scene_on(s, t->scene_frames, t->scene_W, t->scene_H, &scene)) return st;
  const RoughChainArgs c = {d.header, (uint64_t)d.cap_clusters, model->d_jobs, reinterpret_cast<const DepthCrop*>(model->d_crops), model->cap_slots, scene,
                            d.n_frames, t->scene_W, t->scene_H, d.chain_header, d.poses, d.checks, d.keep, d.keep_thresh};
  const dim3 grid((unsigned)d.cap_clusters), block(256);
  const pr::Schedule S = t->schedule_for(PR);
  if (t->plane_for(S)) {
    if (lmx_status st = t->plane_normals_on(s, t->scene_frames, t->scene_W, t->scene_H)) return st;
    hipLaunchKernelGGL(k_rough_refine_clusters<true>, grid, block, 0, s, c, PR, S, t->d_scene_normals, t->plane);
  } else {
    hipLaunchKernelGGL(k_rough_refine_clusters<false>, grid, block, 0, s, c, PR, S, nullptr, t->plane);
  }
  HIP_RETURN(hipGetLastError());
  hipLaunchKernelGGL(k_rough_verify_clusters, grid, block, 0, s, c, PV);
  HIP_RETURN(hipGetLastError());
  HIP_RETURN(hipEventRecord(model->done, s));
  model->done_pending = true;
  return chain_end(t, user, with_user);
}
}  // namespace

extern "C" lmx_status lmx_rough_pose_chain_on(lmx_depth_templates* t, lmx_rough_model* model, const lmx_rough_chain_desc* d, void* stream) {
  return lmx::guarded("lmx_rough_pose_chain_on", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_rough_pose_chain_on";
    if (!t || !model || !d) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    std::lock_guard<std::mutex> lkm(model->m);
    pr::Params PR;
    pv::Params PV;
    if (lmx_status st = rough_check(what, t, model, d, &PR, &PV)) return st;
    if (lmx_status st = t->ensure_device()) return st;
    hipStream_t user = static_cast<hipStream_t>(stream);
    if (lmx_status st = check_user_stream(what, user)) return st;
    const struct { const char* name; const void* p; size_t align; } arrays[] = {
        {"header", d->header, 4}, {"frame_info", d->frame_info, 4}, {"matches", d->matches, 4}, {"clusters", d->clusters, 8}, {"members", d->members, 4},
        {"chain_header", d->chain_header, 4}, {"rough", d->rough, 8}, {"member_group", d->member_group, 4}, {"poses", d->poses, 8}, {"checks", d->checks, 8},
        {"keep", d->keep, 1}};
    for (const auto& arr : arrays)
      if (lmx_status st = check_chain_memory(what, t, arr.name, arr.p, arr.align)) return st;
    const lmx_status st = rough_queue(t, model, *d, PR, PV, user, true);
    if (st != LMX_OK) t->drain_after_error();
    return st;
  });
}

extern "C" lmx_status lmx_debug_rough_pose_chain(lmx_depth_templates* t, lmx_rough_model* model, const lmx_rough_chain_desc* d) {
  return lmx::guarded("lmx_debug_rough_pose_chain", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_debug_rough_pose_chain";
    if (!t || !model || !d) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(t->m);
    std::lock_guard<std::mutex> lkm(model->m);
    pr::Params PR;
    pv::Params PV;
    if (lmx_status st = rough_check(what, t, model, d, &PR, &PV)) return st;
    if (d->cap_matches > ((size_t)1 << 24) || d->cap_members > ((size_t)1 << 24)) { set_error("%s: at most 2^24 matches and members", what); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = t->ensure_device()) return st;
    hipStream_t s = t->s;
    const size_t C = d->cap_clusters;
    // five inputs, six outputs (chain_header is zeroed by the call)
    const HookArray arr[11] = {{d->header, xpack::H_WORDS * sizeof(uint32_t), false}, {d->frame_info, (size_t)d->n_frames * xpack::I_WORDS * sizeof(int32_t), false},
                               {d->matches, d->cap_matches * sizeof(lmx_match_t), false}, {d->clusters, C * sizeof(lmx_cluster_t), false},
                               {d->members, d->cap_members * sizeof(int32_t), false}, {d->chain_header, pc::C_WORDS * sizeof(uint32_t), true},
                               {d->rough, C * sizeof(lmx_rough_pose_t), true}, {d->member_group, d->cap_members * sizeof(int32_t), true},
                               {d->poses, C * sizeof(lmx_pose_refine_t), true}, {d->checks, C * sizeof(lmx_pose_verify_t), true}, {d->keep, C, true}};
    HookArrays<11> h;
    if (lmx_status st = h.upload(arr, s)) return st;
    lmx_rough_chain_desc dd = *d;
    dd.header = h.at<uint32_t>(0); dd.frame_info = h.at<int32_t>(1); dd.matches = h.at<lmx_match_t>(2); dd.clusters = h.at<lmx_cluster_t>(3);
    dd.members = h.at<int32_t>(4); dd.chain_header = h.at<uint32_t>(5); dd.rough = h.at<lmx_rough_pose_t>(6); dd.member_group = h.at<int32_t>(7);
    dd.poses = h.at<lmx_pose_refine_t>(8); dd.checks = h.at<lmx_pose_verify_t>(9); dd.keep = h.at<uint8_t>(10);
    const lmx_status st = rough_queue(t, model, dd, PR, PV, nullptr, false);
    if (lmx_status e = h.finish(s, st == LMX_OK)) return e;
    t->export_read_pending = false;
    model->done_pending = false;
    return st;
  });
}
