// Internal declarations shared by the host side (lmx_ctx.hpp lists its translation units) and the HIP kernels
// (lmx_kernels.hip) of liblmx.so.  Nothing here crosses the C ABI (include/lmx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <new>
#include <exception>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "lmx.h"
#include "lmx_bank_tables.hpp"   // the host bank, LevelGeom and the kernels' table entries (no HIP)
#include "lmx_launch_helper.hpp"   // the one-frame call's helper thread (no HIP)

namespace lmx {

void stream_copy(void* dst, const void* src, size_t n);   // lmx_hostcopy.cpp: copy into pinned staging with non-temporal stores
void copy_rows(void* dst, const void* src, size_t row_bytes, size_t src_stride, int rows);   // lmx_hostcopy.cpp: rows of an image to packed rows, one stream_copy when it is dense
void stream_store_flag(uint32_t* flag, uint32_t value);    // lmx_hostcopy.cpp: the progress word of a streamed frame store (see StreamWait)
lmx_status yaml_load(const char* path, lmx_bank** out);
lmx_status yaml_save(const lmx_bank* bank, const char* path);
void default_normal_lut(uint8_t* out /* [LMX_NORMAL_LUT_SIZE] */);
// labels -> median bins (0 for "no label", k + 1 for 1 << k): the form the depth kernel reads; false if an entry is not one-hot/0
bool normal_lut_to_bins(const uint8_t* lut, uint8_t* bins);
lmx_status normal_lut_from_file(const char* path, std::vector<uint8_t>& out);

// ---- host thread pool ------------------------------------------------------------------------------------
// Host threads for the staging copies of lmx_ctx_upload (pageable caller memory -> pinned staging): one batch of 64 RGB-D
// frames is 98 MB, which a single thread copies slower than PCIe moves it.  parallel_for hands out task indices through an
// atomic counter; the calling thread works too.  Created on first use (LMX_UPLOAD_THREADS overrides the thread count).
class CopyPool {
 public:
  explicit CopyPool(int n_threads) {
    for (int i = 0; i < n_threads; ++i) workers_.emplace_back([this]() { run(); });
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; ++generation_; }
    cv_.notify_all();
    for (std::thread& t : workers_) t.join();
  }
  void parallel_for(int n_tasks, const std::function<void(int)>& fn) {
    if (n_tasks <= 0) return;
    if (workers_.empty() || n_tasks == 1) { for (int i = 0; i < n_tasks; ++i) fn(i); return; }
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn; n_tasks_ = n_tasks; next_.store(0); busy_ = (int)workers_.size(); ++generation_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(m_);
    done_cv_.wait(lk, [this]() { return busy_ == 0; });
    fn_ = nullptr;
  }
  int threads() const { return (int)workers_.size() + 1; }

 private:
  void work() {
    for (;;) {
      const int i = next_.fetch_add(1);
      if (i >= n_tasks_) break;
      (*fn_)(i);
    }
  }
  void run() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&]() { return generation_ != seen; });
        seen = generation_;
        if (stop_) return;
      }
      work();
      {
        std::lock_guard<std::mutex> lk(m_);
        if (--busy_ == 0) done_cv_.notify_one();
      }
    }
  }
  std::vector<std::thread> workers_;
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int)>* fn_ = nullptr;
  std::atomic<int> next_{0};
  int n_tasks_ = 0, busy_ = 0;
  uint64_t generation_ = 0;
  bool stop_ = false;
};


// The helper thread of the one-frame call (LaunchHelper) lives in lmx_launch_helper.hpp: standard headers only, built and stressed on its own
// by tests/test_launch_helper_host.py.

// ---- hooks for device groups (lmx_group.cpp): several member contexts fed from ONE pinned staging area ------------------
// A group stages a batch of host frames once (layout: modality m at offset sum_{m' < m} frame_bytes[m'] * max_batch, frames
// back to back) and every member DMAs it into its own next frame set.  The members' frame sets advance in lock step, so staging
// area j is only ever read by transfers into set j of each member.
constexpr int32_t LMX_CTX_EXTERNAL_STAGING = 1 << 30;   // lmx_ctx_desc.flags, internal: no per-set pinned staging of its own
int ctx_num_sets(const lmx_ctx* c);
int ctx_next_set(const lmx_ctx* c);
size_t ctx_stage_bytes(const lmx_ctx* c);
size_t ctx_bytes_per_frame(const lmx_ctx* c);                                      // one frame of every modality in the staging layout
lmx_status ctx_check_sources(lmx_ctx* c, int n_frames, const lmx_image* sources, int n_sources, int max_frames /* 0 = the context's max_batch */);
// stride_frames = frames per modality block of the staging area (0 = the context's max_batch; a group with frame groups stages the WHOLE batch
// once and every member transfers its slice [first_frame, first_frame + n_frames) of it, n_frames may be 0)
void ctx_stage_sources(lmx_ctx* c, CopyPool* pool, uint8_t* base, int n_frames, const lmx_image* sources, int stride_frames);
lmx_status ctx_begin_staged_upload(lmx_ctx* c);                                    // host: the next set's previous transfer has left the staging area
lmx_status ctx_finish_staged_upload(lmx_ctx* c, int n_frames, const uint8_t* pinned, int first_frame, int stride_frames);  // queue the DMAs out of `pinned`, make the set current
lmx_status ctx_prepare_graph(lmx_ctx* c, int n_frames, float threshold, bool per_class = false);   // LMX_CTX_HIPGRAPH: capture the next enqueue's chain now if it is not cached (per_class: the chain of lmx_ctx_enqueue_thresholds)
// lmx_ctx_debug_enqueue_labels behind its argument checks: an enqueue whose chain starts at the label images (lmx_enqueue.cpp, enqueue_chain)
lmx_status ctx_enqueue_labels(lmx_ctx* c, int n_frames, const uint8_t* const* labels, float threshold, const float* thresholds, int n_thresholds,
                              const char* const* class_ids, int n_class_ids);
lmx_status ctx_drop_newest(lmx_ctx* c);                                            // undo the most recent enqueue (waits for it, frees its slot)

// Coarse candidate written by k_score_coarse, consumed by k_refine.
struct Candidate {
  uint32_t g;      // shard-local template index (all classes concatenated)
  uint32_t pos;    // raster index r*Wc + c at the coarsest level
  uint32_t raw;    // raw similarity (sum of responses)
  uint32_t frame;  // frame of the batch (candidates of all frames share one list)
};

// Per-class match thresholds (lmx_ctx_enqueue_thresholds): entry k belongs to class index k.  One 8-byte entry, so that one scalar load
// brings both values; `frac` is threshold / 100.f divided in float on the host, what launch_score_coarse hands the uniform kernels.
struct ClassThreshold {
  float threshold;
  float frac;
};

// The candidate list of one output slot, filled by the scoring kernel and read by k_refine.  Appending through ONE counter costs
// 11.3 ns per reservation however many waves there are: device-scope atomics on one 128-byte line serialise (and counters a few bytes
// apart share the line; profiles/r03_atomic_append_microbench.txt), which on rendered banks -- thousands of candidates per frame -- was
// most of the scoring kernel's time.  So the list is striped: kCandStripes counters, each on a line of its own, in front of the slot's
// 64-byte header; a wave reserves all candidates of a chunk with one atomic on the stripe (its id + its append number) mod
// kCandStripes.  Stripe s owns entries [s * SC, (s + 1) * SC), SC = cap / kCandStripes; what does not fit its stripe goes to a spill
// region of `cap` entries behind the stripes through counter kCandStripes.  A stripe counter counts every candidate sent to it, fitted
// or spilled, so  sum of the stripe counters = the number of candidates, and when that is <= cap nothing was dropped (the spill region
// alone holds cap): the overflow rule "candidates > cap" is the one a single list had.  k_refine walks stripes and spill in order and
// writes the total to header word 0, where publish / export / the host find it.  The first workgroup of a batch's first kernel zeroes
// the counters together with the header (`clear16`).
constexpr int kCandStripes = 64;
constexpr int kStripeWords = 32;   // dwords between two counters: one 128-byte line each
constexpr size_t kStripeAreaBytes = (size_t)(kCandStripes + 1) * kStripeWords * 4;
inline size_t cand_list_entries(uint32_t cap) { return (size_t)cap * 2; }   // stripes (n * (cap / n) <= cap for any stripe count n) + spill
inline uint32_t* stripes_of_header(uint32_t* header) { return header - (size_t)(kCandStripes + 1) * kStripeWords; }
inline const uint32_t* stripes_of_header(const uint32_t* header) { return header - (size_t)(kCandStripes + 1) * kStripeWords; }

// Exception barrier of the C ABI: nothing may unwind into a C caller.  The readers size containers from what a file says, so a damaged
// or hostile file can make them throw (std::bad_alloc, std::length_error); the entry points that parse files, build banks and contexts
// or size vectors from device counters run their bodies through this (found by scripts/fuzz_files.py: a mutant of a renderer-params file
// ended the process with std::terminate).
template <typename F>
inline lmx_status guarded(const char* what, F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    set_error("%s: out of memory (a size in the input is implausibly large?)", what);
    return LMX_ERR_INVALID_ARG;
  } catch (const std::exception& e) {
    set_error("%s: %s", what, e.what());
    return LMX_ERR_INVALID_ARG;
  } catch (...) {
    set_error("%s: unknown exception", what);
    return LMX_ERR_INVALID_ARG;
  }
}

// A HIP call of an entry point that holds nothing a return would leak: the error text, then LMX_ERR_NO_DEVICE or LMX_ERR_HIP.
#define HIP_RETURN(expr)                                                                           \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      lmx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
      return e_ == hipErrorNoDevice ? LMX_ERR_NO_DEVICE : LMX_ERR_HIP;                             \
    }                                                                                              \
  } while (0)

// The caller's stream of an entry point that orders its work against it (lmx_ctx.cpp): refused when it is no stream, and while it is
// being captured into a graph (the calls record and wait for events of their own streams).  Null is the default stream.
lmx_status check_user_stream(const char* what, hipStream_t user);

#if defined(__HIPCC__)
// Reductions over the wave's 64 lanes: lane 0 gets the result (the others partial ones; __shfl(.., 0, 64) tells every lane).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_down(v, off, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_down(v, off, 64); v = o > v ? o : v; }
  return v;
}
#endif

struct DeviceBankView {
  int32_t G;                        // templates in this shard
  int32_t L, M;
  const TemplateInfo* info;         // [G]
  const TemplateLevelInfo* linfo;   // [G][L]
  const uint32_t* coarse_off;       // [G][M][kFeatStride] offsets at level L-1, padded with zero_off
  const FeatEntry* feat;            // [L][G][M][kFeatStride] (levels 0..L-2 used by refine)
  const uint8_t* feat_count;        // [L][G][M]
  int32_t nf_max_coarse;            // max features over (g,m) at level L-1
  // Unified table of the coarsest level for the u8 scoring kernel: [G][kFeatStride] entries of ALL modalities of a template,
  // interleaved in groups of 3 (round robin over the modalities), each entry = (dword index << 3 | nibble shift) relative to
  // modality 0's memories of the frame (modality m's memories lie m * uni_mod_block_bytes behind them).  Valid (uni_ok) when
  // every template has at most 63 features at that level in total, so that a placement's sum (<= 252) fits a byte.
  const uint32_t* coarse_uni;
  // The same features as 16-dword blocks for the scalar side (k_score_coarse_sb): [G][SB_MAX_BLOCKS][SB_BLOCK]; per block 15 byte
  // offsets (5 groups x 3 features that share their funnel shift; < 3 leftovers of a shift class are padded with zero-run
  // entries), then one dword with the five shifts (5 bits each) and, from bit 25, the real features consumed so far.
  const uint32_t* coarse_blk;
  const ScoreInfo* sinfo;           // [G]
  int32_t uni_ok;
  int32_t score_variant;            // 0 generic, 1 u8, 2 sb: chosen when the context is created (LMX_SCORE_KERNEL), used when uni_ok
  int32_t score_no_prune;           // LMX_SCORE_NO_PRUNE (read when the context is created): the scoring kernel skips its exact early exits and does
                                    // similarity()'s full work -- identical candidates, data-independent cost (bench.py extra.score_full_work)
  uint32_t uni_mod_block_bytes;     // distance between consecutive modalities' nibble memories (max_batch * nib_mod_stride)
};

struct FrameBuffers {               // device pointers, frame-major with fixed per-frame strides
  uint8_t* lm[kMaxLevels][kMaxModalities];     // byte linear memories (coarsest level only), stride geom[l].mod_stride per frame
  uint8_t* ls[kMaxLevels][kMaxModalities];     // linearised spread images (finer levels), stride geom[l].ls_stride per frame
  uint8_t* quant[kMaxLevels][kMaxModalities];  // quantized label images, stride W_l*H_l per frame
  uint8_t* lmn[kMaxModalities];                // nibble-packed memories of the coarsest level, stride nib_mod_stride
};

struct KernelParams {
  LevelGeom geom[kMaxLevels];
  FrameBuffers fb;
};

// kernel ids for profiling
enum KernelId {
  K_PRE = 0,  // node-side pre-processing: k_pre_color / k_pre_depth with lmx_ctx_upload_raw, k_ingest with lmx_ctx_upload_device
  K_COLOR_QUANTIZE,
  K_DEPTH_QUANTIZE,
  K_NN_DOWN,
  K_SPREAD_LINEARIZE,
  K_PACK_NIBBLES,
  K_SCORE_COARSE,
  K_REFINE,
  K_COUNT
};

// The depth quantiser's table on the device: the bank's NORMAL_LUT as median bins plus ONE trailing zero entry, the address of every pixel whose
// bin is 0 without a look-up (far, no valid neighbours, index past the table) -- the kernel's look-up is then an unconditional load.
constexpr size_t kNormalBinsDeviceBytes = (size_t)LMX_NORMAL_LUT_SIZE + 1;
// that table for a NORMAL_LUT of labels (normal_lut_to_bins + the trailing zero); false if an entry is not one-hot/0
bool normal_bins_device_image(const uint8_t* lut, std::vector<uint8_t>& out /* resized to kNormalBinsDeviceBytes */);

// Streamed input of the one-frame call (lmx_match with a fresh host frame, the reference's own pattern: ..._service.cpp:339-344).  The
// quantisers of level 0 are launched BEFORE the host has written the frame into the frame set's host-visible device buffer; the calling thread
// then stores the rows band by band (non-temporal stores through the PCIe BAR) and publishes, after each band, how many rows have landed in a
// flag word that travels the same posted-write path (so it cannot overtake the rows).  A workgroup waits for the rows its tile reads -- thread 0
// polls the flag with system-scope acquire loads, the rest of the workgroup sits at a barrier -- and the kernel's launch latency and the
// transfer overlap instead of adding up.  The wait is BOUNDED (wall clock): if the rows never arrive the workgroup sets *fail and leaves without
// touching its tile, the chain behind it runs on whatever the buffers hold, and collect() reports the batch as failed instead of hanging.
//   flag word = seq << 20 | rows stored so far (all frames of the batch counted through); seq tells this call's stores from the previous call's
// Two threads may store one modality from both ends (round 4: the colour frame first, by both, then the depth frame): the second word
// `flag_hi` = seq << 20 | first row of the part stored from the bottom.  A tile reading rows [lo, hi) may start when hi <= rows from the top,
// or lo >= first row from the bottom, or the two fronts have met.
struct StreamWait {
  const uint32_t* flag = nullptr;   // device-visible (the frame set's fine-grained buffer); null = the frames are already there
  const uint32_t* flag_hi = nullptr;  // null = stored from the top only
  uint32_t seq = 0;
  uint32_t timeout_ticks = 0;       // of the 100 MHz wall clock
  uint32_t* fail = nullptr;         // set to 1 on a timeout: word 6 of the output slot's header
};

// ---- launchers (lmx_kernels.hip) -------------------------------------------------------------------------
void launch_color_quantize(hipStream_t s, const uint8_t* bgr, uint8_t* quant, uint8_t* pyr_next /* may be null */, int H, int W,
                           int n_frames, float weak_threshold, float* mag_out = nullptr /* trainer: squared magnitude per pixel */,
                           uint32_t* clear16 = nullptr /* 16 dwords zeroed by the first workgroup: the output slot's header */,
                           const StreamWait* wait = nullptr /* small batches: the frame is still being stored by the host */,
                           int n_ch = 3 /* colour planes of bgr and pyr_next: 3, or 1 for a gray context (LMX_CTX_GRAY) */,
                           int forced_tile = 0 /* tile height 16 | 32 pinned by the context's LMX_COLOR_TILE; 0 = chosen by batch size */);
lmx_status train_add_template(lmx_bank* bank, int device, const lmx_image* sources, int n_sources, const char* class_id,
                              const lmx_image* object_mask, int32_t* template_id, int32_t* bounding_box);
void launch_depth_quantize(hipStream_t s, const uint16_t* depth, uint8_t* quant, uint8_t* quant_half, int H, int W, int n_frames, int distance_threshold,
                           int difference_threshold, const uint8_t* lut_bins /* device, [LMX_NORMAL_LUT_SIZE] median bins */,
                           uint32_t* clear16 = nullptr);
// device form of "finalise + cluster" (lmx_f2.hip)
// What a cluster's score is the mean of: the one name of a chain variant, from the public `score` field of lmx_export_clusters_desc (the
// same 0 / 1 / 2) down to the kernels' template argument
enum F2Score : int32_t { F2_SIMILARITY = 0, F2_DEPTH = 1, F2_DEPTH_NORMAL = 2 };
inline F2Score f2_score(bool depth, bool normal) { return depth ? (normal ? F2_DEPTH_NORMAL : F2_DEPTH) : F2_SIMILARITY; }
constexpr int F2_MAX = 2048;   // records per frame the LDS path takes; larger frames go to the large-frame kernels (F2_LARGE_MAX) or the host
// One class's side-car as the CLASSES forms read it; n_templates 0: the class has none, its matches are listed and belong to no cluster
constexpr int F2_CLASSES = 16;
struct F2Class {
  const double* dists;
  const int32_t* rects;
  uint32_t n_templates;
  int32_t step, size_thresh, reserved;
  double radius_min, radius_step;
};
struct F2Params {
  const lmx_raw_match_t* recs;   // the slot's records (all frames of the batch)
  const uint32_t* hdr;           // the slot's header: [1] = records written
  uint32_t cap;
  int32_t n_frames;
  lmx_match_t* out_matches;      // [n_frames][F2_MAX] final matches (std::sort + std::unique applied)
  uint32_t* out_counts;          // [n_frames][4]: final matches, clusters, members, status (0 ok, 1 too many records, 2 side-car/range)
  lmx_cluster_t* out_clusters;   // [n_frames][F2_MAX]
  int32_t* out_members;          // [n_frames][F2_MAX]
  uint8_t* scratch;              // [n_frames][F2_MAX] x 32 bytes: per-cluster score, range, rect
  const double* dists;           // side-car: obj_origin_dists[n_templates]
  const int32_t* rects;          // side-car: rects[n_templates][4]
  uint32_t n_templates;
  int32_t step, size_thresh, do_clusters;
  double radius_min, radius_step;
  // F2_DEPTH and F2_DEPTH_NORMAL only: a cluster's score is the mean of dv::value(diff, no_value) over its members
  const lmx_depth_diff_t* diffs;     // per raw record of the slot (the record walk of lmx_verify.hip), device memory
  lmx_depth_diff_t* out_diffs;       // [n_frames][F2_MAX] in final-match order, next to out_matches (written, never read: may be mapped host memory)
  lmx_depth_diff_t* diff_scratch;    // [n_frames][2][F2_MAX] device memory: a frame's diffs by insertion position, then by final position
  double no_value;
  // F2_DEPTH_NORMAL only: the same three for the normal sums; the score is the mean of nv::value(diff, ndiff, no_value)
  const lmx_normal_diff_t* ndiffs;
  lmx_normal_diff_t* out_ndiffs;
  lmx_normal_diff_t* ndiff_scratch;
  // the CLASSES forms only: a side-car per class instead of dists .. radius_step above, and each cluster's class
  const F2Class* classes;            // [F2_CLASSES], device memory
  int32_t* out_cluster_class;        // [n_frames][F2_MAX], next to out_clusters
};
// k_f2_finalize_cluster<score, classes>, one workgroup per frame; classes: the per-class chain (lmx_ctx_collect_clusters_classes)
void launch_f2(hipStream_t s, const F2Params& p, F2Score score, bool classes);

// The large-frame form of the same chain (k_f2_large, lmx_f2.hip): frames of up to F2_LARGE_MAX raw records, one workgroup of 1024
// threads per LISTED frame, every per-record row in that frame's part of a device-memory workspace (a record costs 8 bytes of LDS in the
// kernels above; 16384 of them do not fit).  A frame's part holds its outputs and the kernel's scratch rows at the offsets of
// F2LargeLayout; the host reads back what the count words say.
constexpr int F2_LARGE_MAX = 16384;
struct F2LargeLayout {   // byte offsets into one frame's part of the workspace; rows of F2_LARGE_MAX elements
  uint32_t matches, clusters, members, cluster_class, diffs, ndiffs;   // outputs (diffs / ndiffs: the scored / normal forms only)
  uint32_t key, spill, sim, tid, rec, x, y, cls, perm, keep, seg, rpos, c_score, c_range, c_rect;
  uint32_t bytes;        // one frame's part, a multiple of 256
};
inline F2LargeLayout f2_large_layout(F2Score score) {
  F2LargeLayout l{};
  uint32_t at = 0;
  auto row = [&](uint32_t elem) { const uint32_t o = at; at += (uint32_t)F2_LARGE_MAX * elem; return o; };
  l.matches = row(sizeof(lmx_match_t)); l.clusters = row(sizeof(lmx_cluster_t)); l.members = row(4); l.cluster_class = row(4);
  l.diffs = score != F2_SIMILARITY ? row(sizeof(lmx_depth_diff_t)) : 0; l.ndiffs = score == F2_DEPTH_NORMAL ? row(sizeof(lmx_normal_diff_t)) : 0;
  l.key = row(8); l.spill = row(8); l.c_score = row(8); l.c_range = row(8); l.c_rect = row(16);
  l.sim = row(4); l.tid = row(4); l.rec = row(4);
  l.x = row(2); l.y = row(2); l.cls = row(2); l.perm = row(2); l.keep = row(2); l.seg = row(2); l.rpos = row(2);
  l.bytes = (at + 255u) & ~255u;
  return l;
}
struct F2LargeParams {
  F2Params p;              // recs .. no_value and classes as above; out_counts is [n listed frames][4] (status as above, never 1 for a frame of
                           // <= F2_LARGE_MAX records); the other out_* pointers and the scratch pointers are not used
  const int32_t* frames;   // [grid] the frames to finish, device memory; workgroup i takes frames[i] and part i of the workspace
  uint8_t* ws;             // [grid][lay.bytes] device memory
  F2LargeLayout lay;
  const uint32_t* n_listed = nullptr;   // device memory, optional: workgroups at or above *n_listed leave at once (a list built on the device,
                                        // lmx_export.hip); null: the grid is exact
};
void launch_f2_large(hipStream_t s, const F2LargeParams& p, int n_listed, F2Score score, bool classes);

// lmx_ctx_export_matches_on (lmx_export.hip; the arithmetic is lmx_export_pack.hpp): everything is device memory
struct ExportParams {
  const lmx_raw_match_t* recs;   // the slot's records and header, as F2Params
  const uint32_t* hdr;
  uint32_t cap;
  int32_t n_frames, max_large;
  // what the chain's kernels wrote: the export's rows and counts, the large-frame workspace (f2_large_layout(F2_SIMILARITY)) and its counts
  const lmx_match_t* rows_matches;       // [n_frames][F2_MAX]
  const lmx_cluster_t* rows_clusters;
  const int32_t* rows_members;
  const uint32_t* counts;                // [n_frames][4]
  const uint8_t* large_ws;               // [max_large][lay.bytes]
  const uint32_t* large_counts;          // [max_large][4]
  F2LargeLayout lay;
  int32_t* large_frames;                 // [max_large] written by k_export_plan, with the count word
  uint32_t* large_listed;
  // the caller's arrays
  uint32_t* header;                      // [16]
  int32_t* frame_info;                   // [n_frames][8]
  lmx_match_t* matches; uint64_t cap_matches;
  lmx_cluster_t* clusters; uint64_t cap_clusters;
  int32_t* members; uint64_t cap_members;
  // lmx_ctx_export_clusters_on only (null otherwise): the rows next to rows_matches / rows_clusters (in a large frame's part: lay.diffs,
  // lay.ndiffs, lay.cluster_class) and the caller's arrays parallel to `matches` / `clusters`
  const lmx_depth_diff_t* rows_diffs;
  const lmx_normal_diff_t* rows_ndiffs;
  const int32_t* rows_cluster_class;
  lmx_depth_diff_t* diffs;
  lmx_normal_diff_t* ndiffs;
  int32_t* cluster_class;
};
void launch_export_plan(hipStream_t s, const ExportParams& e);   // max_large > 0 only
void launch_export_pack(hipStream_t s, const ExportParams& e);
void launch_debug_block_sort_large(hipStream_t s, const float* sim, const int* tid, int n, int* perm, uint8_t* ws /* f2_large_layout(F2_SIMILARITY).bytes */);

// ---- depth check against a resident scene (lmx_verify.hip), for the scored consumer chain (lmx_collect.cpp, lmx_debug.cpp) --------------
struct DepthSceneInfo { int32_t device, count, n_frames, W, H, normals; };   // n_frames 0: no scene uploaded; normals: enable_normals was called
std::mutex& depth_templates_mutex(lmx_depth_templates* t);
DepthSceneInfo depth_templates_scene(const lmx_depth_templates* t);   // everything below: the object's mutex is the caller's to hold
// lmx_depth_templates_upload_scene without taking the mutex (depth must not be null)
lmx_status depth_upload_scene(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames);
// The one launch site of the crop walk (k_walk / k_walk_records_dev): d_diffs[i] (with d_ndiffs: both terms, d_ndiffs[i] too) for item i.
// The items are one of
//   jobs            lmx_verify.hip's own match-list path: n jobs on the object's stream, against the n_frames W x H frames their call staged
//   recs, n         RAW records counted by the host against the uploaded scene: `s` waits for the scene's copies; no launch for n = 0
//   recs, hdr, cap  the same for a caller that has not read the slot's header (lmx_ctx_export_clusters_on): a fixed grid of persistent
//                   workgroups takes the count from hdr[1] on the device and walks nothing when hdr says that a list overflowed `cap`;
//                   room for `cap` results.  Launches always.  `s` also waits for every earlier such walk of the object, and the object
//                   remembers an event behind this one: what changes the crops, the scene or the normals waits for it
// A record is a job by class_index (-1: every class), or with d_class_base (n_classes + 1 entries, device memory) for an object that
// holds several classes' crops (lmx_depth_templates_append): class c's template i is crop class_base[c] + i; a class >= n_classes, a
// template_id outside [0, class_base[c + 1] - class_base[c]) or a frame outside the scene gets zeros and is never walked.
// With d_ndiffs the scene's normals are computed on `s` first if nobody has.
struct DepthJob;
struct DepthWalk {
  const DepthJob* jobs = nullptr;
  int32_t n_frames = 0, W = 0, H = 0;   // jobs only; records take the uploaded scene's
  const lmx_raw_match_t* recs = nullptr;
  uint32_t n = 0;                       // jobs, or records counted by the host
  const uint32_t* hdr = nullptr;        // non-null: the records are counted on the device
  uint32_t cap = 0;
  int32_t grid = 0;                     // device count only: workgroups; 0: the object's (a multiple of the device's compute units)
  int32_t class_index = -1;
  const int32_t* d_class_base = nullptr;
  int32_t n_classes = 0;
  lmx_depth_diff_t* d_diffs = nullptr;
  lmx_normal_diff_t* d_ndiffs = nullptr;   // null: the depth term alone
};
lmx_status depth_launch_walk(lmx_depth_templates* t, hipStream_t s, const DepthWalk& w);
// host matches of scene frame `frame` through the job walk (synchronous); other classes and template ids outside the table get zeros
// (nout: the normal sums too)
lmx_status depth_diff_resident(lmx_depth_templates* t, const lmx_match_t* matches, size_t n, int32_t frame, int32_t class_index, lmx_depth_diff_t* out,
                               lmx_normal_diff_t* nout = nullptr);
// the same under the classed predicate; class_base: n_classes + 1 entries on the host
lmx_status depth_diff_resident_classes(lmx_depth_templates* t, const lmx_match_t* matches, size_t n, int32_t frame, const int32_t* class_base, int32_t n_classes,
                                       lmx_depth_diff_t* out, lmx_normal_diff_t* nout = nullptr);
void launch_debug_block_sort(hipStream_t s, const float* sim, const int* tid, int n, int* perm, unsigned long long* spill);

struct PullEntry { uint64_t src; uint64_t row_stride; };  // one caller-owned pinned image (device-visible address)
void launch_pull_frames(hipStream_t s, const PullEntry* tab /* device-visible */, uint8_t* dst, size_t frame_bytes, int rows, uint32_t row_bytes,
                        int n_frames);
// lmx_ctx_upload_device (lmx_ingest.hip): one modality's frames from the caller's device images `tab` into a frame set; mode = ingest::Mode
namespace ingest { struct Args; }
void launch_ingest(hipStream_t s, int mode, const ingest::Args& a, const PullEntry* tab /* device-visible */, int n_frames);
void launch_publish_records(hipStream_t s, void* dst, const void* src, uint32_t max_records, uint32_t cand_cap);
void launch_copy_bytes(hipStream_t s, void* dst, const void* src, size_t bytes);
void launch_publish_blocks(hipStream_t s, void* dst, const void* src, int n_blocks, size_t block_bytes, uint32_t max_records);
constexpr int kPullMax = 16;
struct PullSources { const void* src[kPullMax]; };   // passed by value: the source blocks of k_pull_blocks
void launch_pull_blocks(hipStream_t s, void* dst, const PullSources& srcs, int n_blocks, size_t block_bytes, uint32_t max_records);
void launch_nn_down2(hipStream_t s, const uint8_t* src /* Hs x Ws */, uint8_t* dst /* Hd x Wd = Hs / 2 x Ws / 2 */, int Hs, int Ws, int Hd, int Wd, int n_frames);
void launch_apply_mask(hipStream_t s, uint8_t* quant, const uint8_t* mask0, int Hl, int Wl, int W0, int H0, int level, int n_frames);
bool spread_writes_nibbles(const LevelGeom& g);
int score_kernel_variant(const DeviceBankView& bank);
void launch_spread_linearize(hipStream_t s, const uint8_t* quant, uint8_t* lm /* coarsest level, byte form */, uint8_t* ls /* finer levels */,
                             uint8_t* lmn /* coarsest level, nibble form */, const LevelGeom& g, int n_frames);
// All modalities of one level in ONE launch (the same kernels, blockIdx.y = modality).  Returns false when the level has no
// fast kernel (generic T / widths): the caller then launches per modality with launch_spread_linearize.
struct SpreadBatch {
  const uint8_t* quant[kMaxModalities];
  uint8_t* lm[kMaxModalities];
  uint8_t* ls[kMaxModalities];
  uint8_t* lmn[kMaxModalities];
};
bool launch_spread_linearize_all(hipStream_t s, const SpreadBatch& b, int n_modalities, const LevelGeom& g, int n_frames);
void launch_pre_color(hipStream_t s, const uint8_t* src, uint8_t* dst, int SH, int SW, int SC, int H, int W, int crop_x, int crop_y, int blur3,
                      int n_frames, int dst_ch /* 3: BGR frame; 1: gray frame (LMX_CTX_GRAY, SC must be 1) */);
void launch_pre_depth(hipStream_t s, const void* src, uint16_t* dst, int SH, int SW, int H, int W, int crop_x, int crop_y, int is_float,
                      int n_frames);
void launch_debug_orientation_label(hipStream_t s, const short* dx, const short* dy, uint8_t* out, size_t n);
// Test hook of the depth quantiser's float stage: the bin before the median of n tap tuples, through the production device functions.
// `patches` holds the tuples so that those functions' addressing resolves (layout: kDebugDepthPatch* below); variant = LMX_DBG_DEPTH_*.
constexpr int kDebugDepthPatchW = 3;        // row stride: the nine taps p1 + 5 (j W + i), i, j in {-1, 0, 1}, are p1 - 20, - 15, .. + 20
constexpr int kDebugDepthPatchGroup = 5;    // five tuples interleave into one run of 45 elements: tuple c's p1 = 45 (c / 5) + c % 5 + 20
constexpr int kDebugDepthPatchElems = 45;
void launch_debug_depth_normal_bins(hipStream_t s, const uint16_t* patches, size_t n, int distance_threshold, int difference_threshold, int variant,
                                    const uint8_t* lut_bins /* device, kNormalBinsDeviceBytes */, uint8_t* out);
void launch_pack_nibbles(hipStream_t s, const uint8_t* lm, uint8_t* lmn, const LevelGeom& g, int n_frames);
void launch_score_coarse(hipStream_t s, const DeviceBankView& bank, const LevelGeom& g, const uint8_t* const* lm_mod /*[M] device ptrs*/,
                         int n_frames, float threshold, const int32_t* class_slot, Candidate* cands /* cand_list_entries(cap) */,
                         uint32_t* header /* the slot's; its stripe counters lie in front of it (stripes_of_header) */, uint32_t cap,
                         int n_stripes /* power of two <= kCandStripes, the same for launch_refine */,
                         const ClassThreshold* class_thr = nullptr /* device, [n_classes]: the per-class kernels, `threshold` is not read */);
// Returns false when nothing was launched (empty shard).  pub_dst != null: the kernel also publishes the slot (header + counted
// records, <= pub_max) to pub_dst when its last workgroup finishes; pub_counter is that slot's zero-initialised ticket counter.
bool launch_refine(hipStream_t s, const DeviceBankView& bank, const KernelParams& kp, int n_frames, float threshold,
                   const int32_t* class_slot, const Candidate* cands, uint32_t* header, uint32_t cap, int n_stripes,
                   lmx_raw_match_t* matches, uint32_t* match_count, void* pub_dst = nullptr, const void* pub_src = nullptr, uint32_t* pub_counter = nullptr,
                   uint32_t pub_max = 0, uint32_t pub_seq = 0 /* written to word 7 of the published header LAST: the host may poll it instead of the slot's event */,
                   const ClassThreshold* class_thr = nullptr /* as for launch_score_coarse */);
// Fused launches of the small-batch chain (lmx_enqueue.cpp issue_small): depth quantiser of level 0 + colour quantiser of level 1, and the
// spread of both levels of a two-level bank.
bool launch_small_depth_color(hipStream_t s, const uint16_t* depth, uint8_t* dq, uint8_t* dq_half, int H, int W, int distance_threshold, int difference_threshold,
                              const uint8_t* lut_bins, const uint8_t* col1, uint8_t* cq1, uint8_t* pyr2, int H1, int W1, float weak_threshold, int n_frames,
                              const StreamWait* wait = nullptr /* the depth frame is still being stored by the host */,
                              int n_ch = 3 /* colour planes of col1 / pyr2 (1: gray context) */);
bool launch_small_spread(hipStream_t s, const SpreadBatch& b0, const LevelGeom& g0, const SpreadBatch& b1, const LevelGeom& g1, int n_mod, int n_frames);

// ---- mesh rasteriser + batched trainer (lmx_mesh.hip, lmx_train.cpp) -----------------------------------------------
namespace mr { struct Camera; struct Tri; }
// Per-view state words the rasteriser kernels keep (int32, one 128-byte line per view)
constexpr int kMeshStateWords = 32;
constexpr int MS_INVALID = 0;        // a vertex at Z <= 0.01: the view is invalid
constexpr int MS_UNION = 1;          // union of the triangles' clamped boxes {x0, y0, x1, y1}: tiles outside it only write zeros
constexpr int MS_LEVEL = 5;          // [kMaxLevels] silhouette boxes {xmin, ymin, xmax, ymax} of the mask at pyramid level l (xmax = -1: empty)
constexpr int MS_CENTRE_DEPTH = 21;  // depth_mm[H / 2][W / 2] (the side-car's D)
constexpr int MS_COUNT = 22;         // the covered pixels of the render (k_rough_raster alone counts them)
// The window of a level the trainer's host half looks at: the silhouette box grown by 2, clamped (train_add_template derives the same on
// the host); an empty mask gives a 4x4 corner, which shows "no candidates" like any other window.
__host__ __device__ inline void mesh_window(const int32_t* box, int w, int h, int* x0, int* y0, int* ww, int* wh) {
  if (box[2] >= 0) {
    *x0 = box[0] - 2 > 0 ? box[0] - 2 : 0; *y0 = box[1] - 2 > 0 ? box[1] - 2 : 0;
    *ww = (box[2] + 3 < w ? box[2] + 3 : w) - *x0; *wh = (box[3] + 3 < h ? box[3] + 3 : h) - *y0;
  } else {
    *x0 = 0; *y0 = 0; *ww = w < 4 ? w : 4; *wh = h < 4 ? h : 4;
  }
}
// One level of a view's slot in the packed read-back: float magnitudes of the ColorGradient modalities, one label plane per modality, the
// level's mask; rounded up to 4 bytes
__host__ __device__ inline size_t mesh_pack_level_bytes(int ww, int wh, int n_mod, int n_cg) {
  return (((size_t)ww * wh * (size_t)(4 * n_cg + n_mod + 1)) + 3) & ~(size_t)3;
}
struct MeshPackArgs {
  const uint8_t* quant[kMaxLevels][kMaxModalities];   // label images, [n_views] frames each (DepthNormal: level 0 only)
  const float* mag[kMaxLevels][kMaxModalities];       // squared magnitudes (ColorGradient) or null (DepthNormal)
  const uint8_t* mask0;
  const int32_t* state;
  uint8_t* out;          // device-visible pinned host memory, slot_bytes per view
  size_t slot_bytes;
  int32_t n_levels, n_mod, n_cg, W, H;
};
void launch_mesh_raster(hipStream_t s, const double* d_tri, int n_tri, const mr::Camera& cam, const double* d_views /* [n_views][10] */, int n_views,
                        int n_levels, mr::Tri* d_work /* [n_views][n_tri] */, int32_t* d_state /* [n_views][kMeshStateWords] */,
                        uint8_t* gray, uint16_t* depth, uint8_t* mask /* [n_views][H][W] each, any may be null */);
void launch_mesh_pack(hipStream_t s, const MeshPackArgs& a, int n_views);
// The device path of the mesh trainer (lmx_train_cand.hip; formats in lmx_train_cand.hpp): per (view, level, modality) the candidate list of
// the window k_mesh_pack would copy.  Lists are reserved on `bump` (zeroed per batch) in `records` (device memory, `cap` records, even).
namespace train_cand { struct ListHeader; struct Record; }
struct TrainCandArgs {
  const uint8_t* quant[kMaxLevels][kMaxModalities];   // as MeshPackArgs
  const float* mag[kMaxLevels][kMaxModalities];       // non-null: the modality is ColorGradient
  const uint8_t* mask0;                               // null: no object mask (lmx_debug_train_extract only)
  const int32_t* state;
  train_cand::ListHeader* headers;                    // device, [n_views][n_levels][n_mod]
  train_cand::Record* records;
  uint32_t* bump;
  uint32_t cap;
  float strong_threshold[kMaxModalities];
  int32_t extract_threshold[kMaxModalities];          // at level 0; halved per level
  int32_t n_levels, n_mod, W, H;
};
void launch_train_candidates(hipStream_t s, const TrainCandArgs& a, int n_views);
// copies records [0, min(*bump, cap)) to `host_dst` (device-visible pinned memory of cap records)
void launch_train_cand_copy(hipStream_t s, const TrainCandArgs& a, train_cand::Record* host_dst);
lmx_status mesh_check_args(const char* what, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam, const lmx_mesh_view* views,
                           int32_t n_views, mr::Camera* out);
int mesh_first_invalid_view(const double* triangles, int32_t n_triangles, const lmx_mesh_view* views, int32_t n_views);

}  // namespace lmx
