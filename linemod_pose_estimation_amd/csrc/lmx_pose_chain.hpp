// What lmx_pose_chain_on (include/lmx.h) decides from the lists an export left in device memory, before any pose arithmetic: which
// cluster slots are live, which frame a slot belongs to, which member leads the cluster, and whether the leader is a job the refine and
// verify bodies may run -- with every index checked before it is used as an address.  Shared by the two kernels of lmx_verify.hip
// (k_pose_refine_clusters, k_pose_verify_clusters) and by plain CPU builds (any compiler but hipcc: tests/cpp/pose_chain_host.cpp), so that
// the rules, hostile lists included, are tested without a GPU.  No pose arithmetic lives here: that stays in lmx_pose_refine.hpp and
// lmx_pose_verify.hpp.
//
// INPUT  header[16], frame_info[n_frames][8], matches, clusters, members as lmx_ctx_export_matches_on (clusters = 1) or
//   lmx_ctx_export_clusters_on wrote them (lmx_export_pack.hpp names the words), and the capacities the caller states for the three arrays.
//
// LIVE RANGE  n_live = min(header[3], cap_clusters).  Slot k < n_live belongs to the frame f whose cluster range holds it:
//   cluster_count > 0 and cluster_begin <= k < cluster_begin + cluster_count.  No such frame: the slot is DEAD.  More than one (ranges that
//   overlap: no export writes them): BROKEN.  The frame's slots are DEAD when its status is not 0, when header[1] has the overflow flag, or
//   when one of its three ranges ends beyond the array's capacity; a negative begin or count is BROKEN.
//
// LEADER  cluster_leaders of detector.py: among members[member_begin .. member_begin + member_count) the member of highest similarity, the
//   first in member order on a tie.  Members index their frame's matches: the leader's index into `matches` is match_begin + member.
//   Similarities are compared through sim_key, a total order on their bits (-0 is 0; a NaN lies above every number, as numpy.argmax has
//   it), so the winner does not depend on the order in which lanes are merged.  BROKEN unless member_count >= 1, member_begin >= 0,
//   member_begin + member_count <= min(header[4], cap_members) and every member lies in [0, match_count).
//
// JOB  the leader's match gives the job, or none: another class than class_index (NO_JOB_CLASS: not an error); a template_id outside the
//   table -- with class_base a class outside [0, n_classes) or an id outside its class's range, as record_class_job of lmx_verify.hip --
//   or a rect corner beyond +-2^17 (NO_JOB_BOUNDS).
//
// OUTPUT per slot below n_live: DEAD and BROKEN give leader -1, the NO_JOB states the leader's index; all four give zeroed pose and
//   verify records and keep 0.  Slots at or above n_live are not written.  Flags (chain_header[1]): FLAG_CUT the export's list overflowed
//   or a capacity (the export's or this call's) cut live slots; FLAG_BOUNDS some slot was BROKEN or NO_JOB_BOUNDS; FLAG_POSE some refined
//   pose failed pv::check_pose.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "lmx_export_pack.hpp"

#if defined(__HIPCC__)
#define LMX_PC_FN __host__ __device__ inline
#else
#define LMX_PC_FN inline
#endif

namespace lmx {
namespace pc {

constexpr uint64_t kMaxClusters = (uint64_t)1 << 20;   // cap_clusters: the first kernel's grid
constexpr int32_t kMaxRectCorner = 1 << 17;            // pr::kMaxCoord / 2, what pose_call enforces on the host
constexpr int kLanes = 64;                             // the wave that runs the prologue

enum Flag : uint32_t { FLAG_CUT = 1, FLAG_BOUNDS = 2, FLAG_POSE = 4 };
enum Header : int { C_LIVE = 0, C_FLAGS, C_REFINED, C_VERIFIED, C_KEPT, C_WORDS = 8 };
enum State : int32_t { DEAD = 0, BROKEN, NO_JOB_BOUNDS, NO_JOB_CLASS, JOB };

struct Match { int32_t x, y; float similarity; int32_t template_id, class_index; };                        // the bytes of lmx_match_t
struct Cluster { int32_t index[3], rect[4]; double score; int32_t member_begin, member_count; };          // the bytes of lmx_cluster_t
static_assert(sizeof(Match) == 20 && sizeof(Cluster) == 48 && offsetof(Cluster, member_begin) == 40, "the exported records");

struct Lists {
  const uint32_t* header;      // [16]
  const int32_t* frame_info;   // [n_frames][8]
  int32_t n_frames;
  const Match* matches;
  const Cluster* clusters;
  const int32_t* members;
  uint64_t cap_matches, cap_clusters, cap_members;
};
struct Table {
  int32_t count;               // templates in the object
  const int32_t* rects;        // [count][4]
  int32_t class_index;         // without class_base: -1 = every class
  const int32_t* class_base;   // null, or [n_classes + 1] ending at count
  int32_t n_classes;
};
// What a slot comes to.  leader: the index into `matches`, or -1.  The job's fields are valid with state JOB only.
struct Slot {
  int32_t state;
  uint32_t flags;
  int32_t leader, frame;
  int32_t x, y, template_id, rect_x, rect_y;   // template_id: the crop's index in the object (rebased by class_base)
};
struct Frame { int32_t frame, match_begin, match_count; };

LMX_PC_FN uint32_t n_live(const uint32_t* header, uint64_t cap_clusters) {
  const uint32_t n = header[xpack::H_CLUSTERS];
  return (uint64_t)n <= cap_clusters ? n : (uint32_t)cap_clusters;   // cap_clusters <= kMaxClusters
}
LMX_PC_FN uint32_t n_live(const Lists& L) { return n_live(L.header, L.cap_clusters); }

// What block 0 reports whatever the slots say: the list overflowed, or clusters lie beyond cap_clusters.
LMX_PC_FN uint32_t header_flags(const Lists& L) {
  return ((L.header[xpack::H_FLAGS] & xpack::FLAG_OVERFLOW) || (uint64_t)L.header[xpack::H_CLUSTERS] > L.cap_clusters) ? (uint32_t)FLAG_CUT : 0u;
}

LMX_PC_FN bool frame_claims(const Lists& L, int32_t f, uint32_t k) {
  const int32_t* info = L.frame_info + (size_t)f * xpack::I_WORDS;
  const int64_t cb = info[xpack::I_CLUSTER_BEGIN], cc = info[xpack::I_CLUSTER_COUNT];
  return cc > 0 && (int64_t)k >= cb && (int64_t)k - cb < cc;
}

// The one frame that claims the slot: may its lists be read?  DEAD / BROKEN with the flag to report, or JOB (so far) with *out filled.
LMX_PC_FN int32_t frame_state(const Lists& L, int32_t f, Frame* out, uint32_t* flags) {
  const int32_t* info = L.frame_info + (size_t)f * xpack::I_WORDS;
  const int64_t mb = info[xpack::I_MATCH_BEGIN], mc = info[xpack::I_MATCH_COUNT], cb = info[xpack::I_CLUSTER_BEGIN], cc = info[xpack::I_CLUSTER_COUNT],
                eb = info[xpack::I_MEMBER_BEGIN], ec = info[xpack::I_MEMBER_COUNT];
  const int32_t status = info[xpack::I_STATUS];
  out->frame = f; out->match_begin = (int32_t)mb; out->match_count = (int32_t)mc;
  if (mb < 0 || mc < 0 || cb < 0 || cc < 0 || eb < 0 || ec < 0) { *flags |= FLAG_BOUNDS; return BROKEN; }
  if (L.header[xpack::H_FLAGS] & xpack::FLAG_OVERFLOW) { *flags |= FLAG_CUT; return DEAD; }
  if (status != xpack::ST_DELIVERED) {
    if (status & (xpack::ST_MATCHES_NO_FIT | xpack::ST_CLUSTERS_NO_FIT)) *flags |= FLAG_CUT;
    return DEAD;
  }
  if ((uint64_t)(cb + cc) > L.cap_clusters || (uint64_t)(eb + ec) > L.cap_members || (uint64_t)(mb + mc) > L.cap_matches) { *flags |= FLAG_CUT; return DEAD; }
  return JOB;
}

// May the cluster's member range be read?
LMX_PC_FN bool cluster_ok(const Lists& L, const Cluster& c) {
  const uint64_t total = L.header[xpack::H_MEMBERS];
  const uint64_t end = total < L.cap_members ? total : L.cap_members;
  return c.member_count >= 1 && c.member_begin >= 0 && (uint64_t)((int64_t)c.member_begin + (int64_t)c.member_count) <= end;
}

LMX_PC_FN uint32_t sim_key(float s) {
  union { float f; uint32_t u; } b;
  b.f = s;
  if (s == 0.0f) b.u = 0u;
  return (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
}

// The best member a lane (or a merge of lanes) has seen.  pos: its position in member order, -1: none yet.  bad: a member outside its frame's matches.
struct Best { uint32_t key; int32_t pos, bad; };

LMX_PC_FN Best best_merge(const Best& a, const Best& b) {
  Best o = a;
  if (b.pos >= 0 && (a.pos < 0 || b.key > a.key || (b.key == a.key && b.pos < a.pos))) o = b;
  o.bad = a.bad | b.bad;
  return o;
}

// Lane `lane` of n_lanes: members lane, lane + n_lanes, ... of the cluster (cluster_ok holds, the frame's match range fits `matches`).
LMX_PC_FN Best best_of_lane(const Lists& L, const Frame& fr, const Cluster& c, int lane, int n_lanes) {
  Best b = {0u, -1, 0};
  for (int32_t p = lane; p < c.member_count; p += n_lanes) {
    const int32_t m = L.members[(size_t)c.member_begin + (size_t)p];
    if (m < 0 || m >= fr.match_count) { b.bad = 1; continue; }
    const Best one = {sim_key(L.matches[(size_t)fr.match_begin + (size_t)m].similarity), p, 0};
    b = best_merge(b, one);
  }
  return b;
}

// The slot of a leader (an index into `matches` inside the frame's range): the job, or why there is none.
LMX_PC_FN void slot_of_leader(const Lists& L, const Table& T, const Frame& fr, int32_t leader, Slot* s) {
  const Match m = L.matches[leader];
  s->leader = leader; s->frame = fr.frame; s->x = m.x; s->y = m.y;
  int32_t id = m.template_id;
  if (T.class_base) {
    if (m.class_index < 0 || m.class_index >= T.n_classes) { s->state = NO_JOB_BOUNDS; s->flags |= FLAG_BOUNDS; return; }
    const int32_t first = T.class_base[m.class_index], end = T.class_base[m.class_index + 1];
    if (m.template_id < 0 || m.template_id >= end - first) { s->state = NO_JOB_BOUNDS; s->flags |= FLAG_BOUNDS; return; }
    id = first + m.template_id;
  } else if (T.class_index >= 0 && m.class_index != T.class_index) {
    s->state = NO_JOB_CLASS;
    return;
  }
  if (id < 0 || id >= T.count) { s->state = NO_JOB_BOUNDS; s->flags |= FLAG_BOUNDS; return; }
  const int32_t rx = T.rects[(size_t)id * 4], ry = T.rects[(size_t)id * 4 + 1];
  if (rx < -kMaxRectCorner || rx > kMaxRectCorner || ry < -kMaxRectCorner || ry > kMaxRectCorner) { s->state = NO_JOB_BOUNDS; s->flags |= FLAG_BOUNDS; return; }
  s->template_id = id; s->rect_x = rx; s->rect_y = ry;
  s->state = JOB;
}

LMX_PC_FN Slot slot_none(int32_t state, uint32_t flags) { return Slot{state, flags, -1, -1, 0, 0, 0, 0, 0}; }

// Slot k < n_live(L), from the frames that claim it (their number and the lowest of them) on: everything but the two reductions over the
// lanes, which the caller supplies -- the kernels with wave shuffles, resolve_slot below with loops.  best(frame, cluster): the merged Best
// of all lanes.  leader_in >= -1: do not pick; take this leader (the verify kernel reads the one the refine kernel wrote) -- -1 or one
// outside the frame's matches gives DEAD without a flag.
template <typename BestFn>
LMX_PC_FN Slot slot_from_claims(const Lists& L, const Table& T, uint32_t k, int32_t claims, int32_t first_frame, bool pick, int32_t leader_in, BestFn&& best) {
  if (claims == 0) return slot_none(DEAD, 0u);
  if (claims > 1) return slot_none(BROKEN, FLAG_BOUNDS);
  Frame fr;
  uint32_t flags = 0;
  const int32_t st = frame_state(L, first_frame, &fr, &flags);
  if (st != JOB) return slot_none(st, flags);
  int32_t leader = leader_in;
  if (pick) {
    const Cluster c = L.clusters[k];
    if (!cluster_ok(L, c)) return slot_none(BROKEN, FLAG_BOUNDS);
    const Best b = best(fr, c);
    if (b.bad || b.pos < 0) return slot_none(BROKEN, FLAG_BOUNDS);
    leader = fr.match_begin + L.members[(size_t)c.member_begin + (size_t)b.pos];
  } else if (leader < fr.match_begin || leader - fr.match_begin >= fr.match_count) {
    return slot_none(DEAD, 0u);
  }
  Slot s = slot_none(JOB, 0u);
  slot_of_leader(L, T, fr, leader, &s);
  return s;
}

// The whole decision on one thread, the lanes of the prologue's wave one after the other and merged in the order of its shuffles.
LMX_PC_FN Slot resolve_slot(const Lists& L, const Table& T, uint32_t k, int n_lanes = kLanes) {
  int32_t claims = 0, first = INT32_MAX;
  for (int32_t f = 0; f < L.n_frames; ++f)
    if (frame_claims(L, f, k)) { claims += 1; first = f < first ? f : first; }
  return slot_from_claims(L, T, k, claims, first, true, -1, [&](const Frame& fr, const Cluster& c) {
    Best lanes[kLanes];
    for (int l = 0; l < n_lanes; ++l) lanes[l] = best_of_lane(L, fr, c, l, n_lanes);
    for (int off = n_lanes / 2; off > 0; off >>= 1)
      for (int l = 0; l < off; ++l) lanes[l] = best_merge(lanes[l], lanes[l + off]);
    return lanes[0];
  });
}

}  // namespace pc
}  // namespace lmx
