// The arithmetic of lmx_ctx_export_matches_on (include/lmx.h): which frames the large-frame kernel takes, where each frame's results come
// from, where they go in the caller's flat arrays, whether they fit, and the status words -- the device form of the per-frame loop at the
// end of collect_clusters_impl (lmx_collect.cpp).  Shared by the kernels of lmx_export.hip and by plain CPU builds (any compiler but hipcc:
// tests/cpp/export_pack_host.cpp), so that the rules are tested without a GPU.  lmx_ctx_export_clusters_on adds the arrays parallel to
// the matches and the clusters: the last section (tests/cpp/export_clusters_pack_host.cpp).
//
// Inputs are the count words the chain's kernels leave behind:
//   counts[f][4]   of k_f2_finalize_cluster, one row per frame: {final matches, clusters, members, status}; status 0 delivered, 1 more than
//                  kSmallMax raw records ([0] is then the number of raw records), 2 a ring outside the packed range ([0] final matches)
//   lcounts[i][4]  of k_f2_large, one row per LISTED frame, the same meaning
// A frame is listed for the large-frame kernel when its row says status 1 with at most kLargeMax records and fewer than max_large frames
// before it were listed: frame order decides, and list_index() gives the same answer to the kernel that builds the list and to the one
// that packs.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LMX_XP_FN __host__ __device__ inline
#else
#define LMX_XP_FN inline
#endif

namespace lmx {
namespace xpack {

constexpr uint32_t kSmallMax = 2048;    // F2_MAX
constexpr uint32_t kLargeMax = 16384;   // F2_LARGE_MAX

// frame_info[f][6]
enum Status : int32_t {
  ST_DELIVERED = 0,
  ST_UNFINISHED = 1,        // too many raw records for the kernels this call could use
  ST_RANGE = 2,             // the chain's own status 2
  ST_MATCHES_NO_FIT = 4,    // or-ed onto ST_DELIVERED
  ST_CLUSTERS_NO_FIT = 8,   // or-ed onto ST_DELIVERED: the clusters or the members
  ST_OVERFLOW = 16,         // the slot's candidate or record list overflowed
};
// header[1]
enum Flag : uint32_t { FLAG_OVERFLOW = 1, FLAG_UNFINISHED = 2, FLAG_NO_FIT = 4 };
// header words
enum Header : int { H_FRAMES = 0, H_FLAGS, H_MATCHES, H_CLUSTERS, H_MEMBERS, H_CANDIDATES, H_RECORDS, H_WORDS = 16 };
// frame_info words
enum Info : int { I_MATCH_BEGIN = 0, I_MATCH_COUNT, I_CLUSTER_BEGIN, I_CLUSTER_COUNT, I_MEMBER_BEGIN, I_MEMBER_COUNT, I_STATUS, I_RAW_RECORDS, I_WORDS = 8 };

struct Caps { uint64_t matches, clusters, members; };

LMX_XP_FN bool list_overflowed(uint32_t n_candidates, uint32_t n_records, uint32_t capacity) { return n_candidates > capacity || n_records > capacity; }

// does the large-frame kernel take a frame with this count row, given room in the list?
LMX_XP_FN bool wants_large(const uint32_t* row) { return row[3] == 1u && row[0] <= kLargeMax; }

// running state over the frames of a batch, in frame order
struct Walk {
  uint64_t matches = 0, clusters = 0, members = 0;   // the totals so far = the next frame's *_begin
  int32_t wanted = 0;                                // frames so far that wants_large()
  uint32_t flags = 0;
};

// where one frame's results lie and go
struct Slot {
  uint64_t match_begin, cluster_begin, member_begin;
  uint32_t n_matches, n_clusters, n_members;
  int32_t status;          // what frame_info reports
  int32_t part;            // >= 0: the results lie in part `part` of the large-frame workspace; -1: in the frame's rows
  bool write_matches;      // the whole range fits cap.matches
  bool write_clusters;     // both the clusters' and the members' range fit
};

// Frame f's place in the large-frame list, or -1.  `wanted_before` = frames g < f with wants_large(counts + 4 g).
LMX_XP_FN int32_t list_index(const uint32_t* row, int32_t wanted_before, int32_t max_large) {
  return wants_large(row) && wanted_before < max_large ? wanted_before : -1;
}

// Advances `w` over frame f (call for f = 0, 1, ... in order) and says where the frame's results lie and go.
LMX_XP_FN Slot step(Walk& w, const uint32_t* counts, const uint32_t* lcounts, int32_t f, int32_t max_large, bool overflowed, const Caps& cap) {
  const uint32_t* row = counts + (size_t)f * 4;
  Slot s;
  s.match_begin = w.matches; s.cluster_begin = w.clusters; s.member_begin = w.members;
  s.n_matches = s.n_clusters = s.n_members = 0;
  s.part = -1; s.write_matches = s.write_clusters = false;
  if (overflowed) {
    s.status = ST_OVERFLOW;
    w.flags |= FLAG_OVERFLOW;
    return s;
  }
  const int32_t part = list_index(row, w.wanted, max_large);
  if (wants_large(row)) w.wanted += 1;
  const uint32_t* src = row;
  if (part >= 0) { src = lcounts + (size_t)part * 4; s.part = part; }
  if (src[3] != 0u) {   // nobody finished the frame
    s.status = src[3] == 2u ? ST_RANGE : ST_UNFINISHED;
    s.part = -1;
    w.flags |= FLAG_UNFINISHED;
    return s;
  }
  s.n_matches = src[0]; s.n_clusters = src[1]; s.n_members = src[2];
  s.write_matches = s.match_begin + s.n_matches <= cap.matches;
  s.write_clusters = s.cluster_begin + s.n_clusters <= cap.clusters && s.member_begin + s.n_members <= cap.members;
  s.status = ST_DELIVERED | (s.write_matches ? 0 : ST_MATCHES_NO_FIT) | (s.write_clusters ? 0 : ST_CLUSTERS_NO_FIT);
  if (s.status != ST_DELIVERED) w.flags |= FLAG_NO_FIT;
  w.matches += s.n_matches; w.clusters += s.n_clusters; w.members += s.n_members;
  return s;
}

// frame_info[f] of a frame with `raw_records` records in the slot
LMX_XP_FN void fill_info(int32_t* info, const Slot& s, uint32_t raw_records) {
  info[I_MATCH_BEGIN] = (int32_t)s.match_begin; info[I_MATCH_COUNT] = (int32_t)s.n_matches;
  info[I_CLUSTER_BEGIN] = (int32_t)s.cluster_begin; info[I_CLUSTER_COUNT] = (int32_t)s.n_clusters;
  info[I_MEMBER_BEGIN] = (int32_t)s.member_begin; info[I_MEMBER_COUNT] = (int32_t)s.n_members;
  info[I_STATUS] = s.status; info[I_RAW_RECORDS] = (int32_t)raw_records;
}

// the header once every frame has been stepped over
LMX_XP_FN void fill_header(uint32_t* header, const Walk& w, int32_t n_frames, uint32_t n_candidates, uint32_t n_records) {
  for (int i = 0; i < H_WORDS; ++i) header[i] = 0u;
  header[H_FRAMES] = (uint32_t)n_frames; header[H_FLAGS] = w.flags;
  header[H_MATCHES] = (uint32_t)w.matches; header[H_CLUSTERS] = (uint32_t)w.clusters; header[H_MEMBERS] = (uint32_t)w.members;
  header[H_CANDIDATES] = n_candidates; header[H_RECORDS] = n_records;
}

// ---- lmx_ctx_export_clusters_on: the arrays that lie parallel to the matches and to the clusters ------------------------------------------
// diffs and ndiffs share the matches' offsets, capacity and fit decision, cluster_class the clusters' (which the members decide too): a
// frame's range of a side array is written iff the call has that array and the frame's range of its parent array is written.
constexpr uint32_t kDiffDwords = 4;   // lmx_depth_diff_t and lmx_normal_diff_t, as the pack kernel copies them

struct SideArrays { bool diffs, ndiffs, cluster_class; };   // which of them the call has

struct SideSlot {
  uint64_t diff_begin;    // = match_begin, in elements of diffs and of ndiffs
  uint32_t n_diffs;       // = n_matches
  uint64_t class_begin;   // = cluster_begin
  uint32_t n_class;       // = n_clusters
  bool write_diffs, write_ndiffs, write_cluster_class;
};

LMX_XP_FN SideSlot side_slot(const Slot& s, const SideArrays& has) {
  SideSlot o;
  o.diff_begin = s.match_begin; o.n_diffs = s.n_matches;
  o.class_begin = s.cluster_begin; o.n_class = s.n_clusters;
  o.write_diffs = has.diffs && s.write_matches;
  o.write_ndiffs = has.ndiffs && s.write_matches;
  o.write_cluster_class = has.cluster_class && s.write_clusters;
  return o;
}

}  // namespace xpack
}  // namespace lmx
