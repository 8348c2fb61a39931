// Kernels of lmx_ctx_export_matches_on (include/lmx.h): the final match list and the clusters of an enqueue, packed into the caller's
// device arrays without a host in the loop.  The chain on the context's export stream, one kernel boundary between any two stages that
// exchange data (no flag, no grid barrier):
//
//   k_f2_finalize_cluster   (lmx_f2.hip) one workgroup per frame into the export's own device rows [F][F2_MAX] and counts [F][4]
//   k_export_plan           one workgroup, lane 0: the frames the count rows hand back with status 1 and at most F2_LARGE_MAX records, in
//                           frame order, up to max_large_frames of them -> frame list + count word.  F <= max_batch rows: a serial walk
//   k_f2_large              (lmx_f2.hip) grid = max_large_frames, workgroups at or above the count word leave at once
//   k_export_pack           one workgroup of 256 per frame: lane 0 walks the count rows of the frames up to its own (xpack::step: offsets, fit,
//                           status; at most max_batch short steps), the workgroup counts the frame's raw records in the slot's list and copies
//                           the frame's matches, clusters (member_begin rebased to the flat member array) and members from its rows or from
//                           its part of the large-frame workspace; lane 0 writes frame_info, and the last frame's workgroup the header.
// lmx_ctx_export_clusters_on runs the same chain with the scored / classed forms of the two lmx_f2.hip kernels (behind the crop walk
// k_walk_records_dev of lmx_verify.hip), and k_export_pack then also copies the frame's diffs and ndiffs (under the matches' fit decision)
// and cluster_class (under the clusters'): xpack::side_slot.
// The arithmetic is lmx_export_pack.hpp, shared with the CPU tests.
#include <hip/hip_runtime.h>

#include "lmx_internal.hpp"
#include "lmx_export_pack.hpp"

namespace lmx {
namespace {

static_assert(xpack::kSmallMax == (uint32_t)F2_MAX && xpack::kLargeMax == (uint32_t)F2_LARGE_MAX, "lmx_export_pack.hpp restates the chain's limits");
static_assert(sizeof(lmx_match_t) == 20 && sizeof(lmx_cluster_t) == 48 && offsetof(lmx_cluster_t, member_begin) == 40, "the pack kernel copies dwords");
static_assert(sizeof(lmx_depth_diff_t) == 4 * xpack::kDiffDwords && sizeof(lmx_normal_diff_t) == 4 * xpack::kDiffDwords, "the pack kernel copies dwords");

constexpr int XP_T = 256;

__global__ __launch_bounds__(64) void k_export_plan(ExportParams e) {
  if (threadIdx.x != 0) return;
  int32_t listed = 0;
  if (!xpack::list_overflowed(e.hdr[0], e.hdr[1], e.cap)) {
    int32_t wanted = 0;
    for (int32_t f = 0; f < e.n_frames; ++f) {
      const uint32_t* row = e.counts + (size_t)f * 4;
      const int32_t at = xpack::list_index(row, wanted, e.max_large);
      if (xpack::wants_large(row)) ++wanted;
      if (at >= 0) { e.large_frames[at] = f; listed = at + 1; }
    }
  }
  *e.large_listed = (uint32_t)listed;
}

// n dwords; 16-byte moves where both sides allow
__device__ __forceinline__ void copy_dwords(uint32_t* dst, const uint32_t* src, uint32_t n, int tid) {
  if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0) {
    const uint32_t n4 = n >> 2;
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    for (uint32_t i = tid; i < n4; i += XP_T) d4[i] = s4[i];
    for (uint32_t i = (n4 << 2) + tid; i < n; i += XP_T) dst[i] = src[i];
  } else {
    for (uint32_t i = tid; i < n; i += XP_T) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(XP_T) void k_export_pack(ExportParams e) {
  __shared__ xpack::Slot s_slot;
  __shared__ uint32_t s_raw;
  const int tid = threadIdx.x, frame = blockIdx.x;
  const uint32_t n_cand = e.hdr[0], n_rec = e.hdr[1];
  const bool overflowed = xpack::list_overflowed(n_cand, n_rec, e.cap);
  if (tid == 0) {
    s_raw = 0;
    xpack::Walk w;
    xpack::Slot s{};
    const xpack::Caps cap{e.cap_matches, e.cap_clusters, e.cap_members};
    for (int32_t f = 0; f <= frame; ++f) s = xpack::step(w, e.counts, e.large_counts, f, e.max_large, overflowed, cap);
    s_slot = s;
    if (frame == e.n_frames - 1) xpack::fill_header(e.header, w, e.n_frames, n_cand, n_rec);
  }
  __syncthreads();
  if (!overflowed) {
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n_rec; i += XP_T) mine += e.recs[i].frame == frame ? 1u : 0u;
    if (mine) atomicAdd(&s_raw, mine);
  }
  __syncthreads();
  const xpack::Slot s = s_slot;
  if (tid == 0) xpack::fill_info(e.frame_info + (size_t)frame * xpack::I_WORDS, s, s_raw);
  // the frame's results: its rows, or its part of the large-frame workspace
  const lmx_match_t* src_m = e.rows_matches + (size_t)frame * F2_MAX;
  const lmx_cluster_t* src_c = e.rows_clusters + (size_t)frame * F2_MAX;
  const int32_t* src_mem = e.rows_members + (size_t)frame * F2_MAX;
  if (s.part >= 0) {
    const uint8_t* part = e.large_ws + (size_t)s.part * e.lay.bytes;
    src_m = reinterpret_cast<const lmx_match_t*>(part + e.lay.matches);
    src_c = reinterpret_cast<const lmx_cluster_t*>(part + e.lay.clusters);
    src_mem = reinterpret_cast<const int32_t*>(part + e.lay.members);
  }
  if (s.write_matches && s.n_matches)
    copy_dwords(reinterpret_cast<uint32_t*>(e.matches + s.match_begin), reinterpret_cast<const uint32_t*>(src_m), s.n_matches * 5u, tid);
  if (s.write_clusters) {
    // a cluster is 12 dwords, member_begin the 11th: rebased to the flat member array, as collect_clusters' host loop does
    uint32_t* dst = reinterpret_cast<uint32_t*>(e.clusters + s.cluster_begin);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(src_c);
    const uint32_t n = s.n_clusters * 12u;
    for (uint32_t i = tid; i < n; i += XP_T) dst[i] = src[i] + (i % 12u == 10u ? (uint32_t)s.member_begin : 0u);
    if (s.n_members)
      copy_dwords(reinterpret_cast<uint32_t*>(e.members + s.member_begin), reinterpret_cast<const uint32_t*>(src_mem), s.n_members, tid);
  }
  // lmx_ctx_export_clusters_on: what lies parallel to the matches and to the clusters
  const xpack::SideSlot o = xpack::side_slot(s, xpack::SideArrays{e.diffs != nullptr, e.ndiffs != nullptr, e.cluster_class != nullptr});
  if (o.write_diffs && o.n_diffs) {
    const lmx_depth_diff_t* src = s.part >= 0 ? reinterpret_cast<const lmx_depth_diff_t*>(e.large_ws + (size_t)s.part * e.lay.bytes + e.lay.diffs)
                                              : e.rows_diffs + (size_t)frame * F2_MAX;
    copy_dwords(reinterpret_cast<uint32_t*>(e.diffs + o.diff_begin), reinterpret_cast<const uint32_t*>(src), o.n_diffs * xpack::kDiffDwords, tid);
  }
  if (o.write_ndiffs && o.n_diffs) {
    const lmx_normal_diff_t* src = s.part >= 0 ? reinterpret_cast<const lmx_normal_diff_t*>(e.large_ws + (size_t)s.part * e.lay.bytes + e.lay.ndiffs)
                                               : e.rows_ndiffs + (size_t)frame * F2_MAX;
    copy_dwords(reinterpret_cast<uint32_t*>(e.ndiffs + o.diff_begin), reinterpret_cast<const uint32_t*>(src), o.n_diffs * xpack::kDiffDwords, tid);
  }
  if (o.write_cluster_class && o.n_class) {
    const int32_t* src = s.part >= 0 ? reinterpret_cast<const int32_t*>(e.large_ws + (size_t)s.part * e.lay.bytes + e.lay.cluster_class)
                                     : e.rows_cluster_class + (size_t)frame * F2_MAX;
    copy_dwords(reinterpret_cast<uint32_t*>(e.cluster_class + o.class_begin), reinterpret_cast<const uint32_t*>(src), o.n_class, tid);
  }
}

}  // namespace

void launch_export_plan(hipStream_t s, const ExportParams& e) {
  hipLaunchKernelGGL(k_export_plan, dim3(1), dim3(64), 0, s, e);
}

void launch_export_pack(hipStream_t s, const ExportParams& e) {
  hipLaunchKernelGGL(k_export_pack, dim3((unsigned)e.n_frames), dim3(XP_T), 0, s, e);
}

}  // namespace lmx
