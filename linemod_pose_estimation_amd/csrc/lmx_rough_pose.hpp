// The rough pose of a cluster (lmx_rough_pose_chain_on, include/lmx.h): the reference's getRoughPoseByClustering
// (src/rgbdDetector.cpp:586-865, orientationCompare at :1246-1261) up to the view that is rendered again -- the members of a cluster grouped
// by the orientation of their views, the largest group, the mean of its rotations through quaternions, of its distances and of its match
// positions.  Shared by k_rough_group (lmx_rough.hip) and by plain CPU builds (LMX_RP_HOST, any compiler: tests/cpp/rough_pose_host.cpp).
// Doubles with + - * / sqrt in the written order only (build with -ffp-contract=off) and integers: gfx950 and a CPU agree bit for bit.
// Everything decided from the exported lists alone is lmx_pose_chain.hpp's (pc::): the live range, the frame of a slot, cluster_ok, the flags.
//
// VIEW TABLE  n_views entries indexed by a match's template_id: R[9] row major, distance, D and ori_dist (the side-car's D and Ori_dist;
//   zeros without them) and the quaternion q = (x, y, z, w) of R, computed once on the host by quat_of: Eigen 3's matrix-to-quaternion,
//     t = (R00 + R11) + R22 > 0:  s = sqrt(t + 1), w = s/2, s' = 0.5/s, x = (R21 - R12)s', y = (R02 - R20)s', z = (R10 - R01)s'
//     otherwise: i = 0; if R11 > R00: i = 1; if R22 > Rii: i = 2; j = (i+1)%3, k = (j+1)%3; s = sqrt(((Rii - Rjj) - Rkk) + 1), q[i] = s/2,
//       s' = 0.5/s, w = (Rkj - Rjk)s', q[j] = (Rji + Rij)s', q[k] = (Rki + Rik)s'
//   Eigen is not part of the reference tree: parity with it is not pinned.
//
// SLOT  k < pc::n_live: DEAD and BROKEN as lmx_pose_chain.hpp has them for the frame and for cluster_ok.  Then, over all members (an OR:
//   no order), before any value is used as an address: a member outside [0, match_count) of its frame: BROKEN.  A member whose class differs
//   from the first member's: BROKEN.  With class_index >= 0 a first member of another class: NO_JOB_CLASS (no flag).  A template_id outside
//   [0, n_views): NO_JOB_BOUNDS.  In that precedence.  After the means: |x| or |y| of the mean position above 2^17: NO_JOB_BOUNDS (the
//   window corner that is added to it lies inside the model camera's image, below 2^14).  BROKEN and NO_JOB_BOUNDS raise pc::FLAG_BOUNDS.
//   Every state but JOB gives an all-zero record.  member_group is written for a slot whose members passed the checks of the lists (the
//   mean-position case included), for no other.
//
// GROUPS  first fit in member order (:595-632): member p joins the first group g, in creation order, whose front -- the member that created
//   it -- has same(R_p, R_front): tr > trace_min with tr = sum over k = 0..8 of R_p[k] * R_front[k], added left to right: the trace of
//   R_p^T R_front = 1 + 2 cos(angle).  trace_min = 1 + 2 cos(threshold): the strict < of the reference's angle test is the strict > here.
//   No group passes: p creates group n_groups.  At most kMaxGroups: the member that would create one more ends the slot with status
//   TOO_MANY_GROUPS (n_members and n_groups = kMaxGroups set, the rest zero); it and the members behind it get member_group -1.
//
// WINNER  what std::sort(groups, by size descending) leaves at index 0: sortemu::sort over the group indices 0 .. n_groups - 1 with
//   less(i, j) = size[i] > size[j].
//
// MEANS  over the winner's members in member order: q added coefficient by coefficient with no sign alignment (:670), divided by the count,
//   n2 = ((xx + yy) + zz) + ww; n2 zero or not finite: status DEGENERATE (R zeros, everything else of the record set); q / sqrt(n2); R by
//   Eigen's toRotationMatrix: tx = 2x, ty = 2y, tz = 2z, twx = tx w, twy = ty w, twz = tz w, txx = tx x, txy = ty x, txz = tz x, tyy = ty y,
//   tyz = tz y, tzz = tz z; R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy, R10 = txy + twz, R11 = 1 - (txx + tzz), R12 = tyz - twx,
//   R20 = txz - twy, R21 = tyz + twx, R22 = 1 - (txx + tyy).  distance, D, ori_dist: double sums / count.  x, y: int64 sums / count by C++
//   truncating division (the reference divides through size_t: equal for sums >= 0).  center_hole = 1 iff some member of the group has
//   |D - ori_dist| < 0.001.  front: the index into `matches` of the member that created the winner.
//
// The record then has status OK; the render (lmx_rough.hip) fills rect and n_model or replaces the status by INVALID_VIEW,
// WINDOW_TOO_LARGE or EMPTY.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "lmx_pose_chain.hpp"
#include "lmx_sort_emul.hpp"

#if defined(__HIPCC__) && !defined(LMX_RP_HOST)
#define LMX_RP_FN __host__ __device__ inline
#else
#define LMX_RP_FN inline
#endif

namespace lmx {
namespace rp {

constexpr int kMaxGroups = 512;
constexpr int32_t kMaxMean = 1 << 17;
constexpr uint32_t FLAG_ROUGH = 8;    // chain_header[1]: a live job slot ended with a status other than OK
constexpr int C_ROUGH_OK = 5;         // chain_header[5]: slots of status OK
enum Status : int32_t { NONE = 0, OK, TOO_MANY_GROUPS, DEGENERATE, INVALID_VIEW, WINDOW_TOO_LARGE, EMPTY };

struct View { double R[9], distance, D, ori_dist, q[4]; };   // q: x, y, z, w
struct Record {                                              // the bytes of lmx_rough_pose_t
  double R[9], distance, D, ori_dist;
  int32_t x, y, n_members, n_groups, group, n_group_members, front, center_hole;
  int32_t rect[4];
  int32_t n_model, status;
};
static_assert(sizeof(View) == 128 && sizeof(Record) == 152 && alignof(Record) == 8 && offsetof(Record, x) == 96 && offsetof(Record, rect) == 128 &&
                  offsetof(Record, status) == 148, "the records");

LMX_RP_FN void quat_of(const double* R, double* q) {
  const double t = (R[0] + R[4]) + R[8];
  if (t > 0.0) {
    const double s = sqrt(t + 1.0), h = 0.5 / s;
    q[3] = 0.5 * s;
    q[0] = (R[7] - R[5]) * h; q[1] = (R[2] - R[6]) * h; q[2] = (R[3] - R[1]) * h;
    return;
  }
  int i = 0;
  if (R[4] > R[0]) i = 1;
  if (R[8] > R[i * 4]) i = 2;
  const int j = (i + 1) % 3, k = (j + 1) % 3;
  const double s = sqrt(((R[i * 4] - R[j * 4]) - R[k * 4]) + 1.0), h = 0.5 / s;
  q[i] = 0.5 * s;
  q[3] = (R[k * 3 + j] - R[j * 3 + k]) * h;
  q[j] = (R[j * 3 + i] + R[i * 3 + j]) * h;
  q[k] = (R[k * 3 + i] + R[i * 3 + k]) * h;
}

LMX_RP_FN double trace_dot(const double* A, const double* B) {
  double tr = A[0] * B[0];
  for (int k = 1; k < 9; ++k) tr = tr + A[k] * B[k];
  return tr;
}

LMX_RP_FN void rot_of_quat(double x, double y, double z, double w, double* R) {
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// ---- the slot, from the lists --------------------------------------------------------------------------------------------------------------
struct Slot { int32_t state; uint32_t flags; int32_t frame, match_begin, match_count, member_begin, member_count; };
struct Scan { int32_t bad_member, bad_view, mixed; };   // ORs over the members: no order

LMX_RP_FN Slot no_slot(int32_t state, uint32_t flags) { return Slot{state, flags, -1, 0, 0, 0, 0}; }

// Lane `lane` of n_lanes: members lane, lane + n_lanes, ... (cluster_ok holds, the frame's match range fits `matches`).
LMX_RP_FN Scan scan_of_lane(const pc::Lists& L, const pc::Frame& fr, const pc::Cluster& c, int32_t n_views, int32_t first_class, int lane, int n_lanes) {
  Scan s = {0, 0, 0};
  for (int32_t p = lane; p < c.member_count; p += n_lanes) {
    const int32_t m = L.members[(size_t)c.member_begin + (size_t)p];
    if (m < 0 || m >= fr.match_count) { s.bad_member = 1; continue; }
    const pc::Match& mm = L.matches[(size_t)fr.match_begin + (size_t)m];
    if (mm.class_index != first_class) s.mixed = 1;
    if (mm.template_id < 0 || mm.template_id >= n_views) s.bad_view = 1;
  }
  return s;
}

// Slot k < n_live from the frames that claim it (their number, the lowest of them) on.  scan(frame, cluster, first_class): the OR of
// scan_of_lane over all lanes.
template <typename ScanFn>
LMX_RP_FN Slot slot_from_claims(const pc::Lists& L, int32_t class_index, uint32_t k, int32_t claims, int32_t first_frame, ScanFn&& scan) {
  if (claims == 0) return no_slot(pc::DEAD, 0u);
  if (claims > 1) return no_slot(pc::BROKEN, pc::FLAG_BOUNDS);
  pc::Frame fr;
  uint32_t flags = 0;
  const int32_t st = pc::frame_state(L, first_frame, &fr, &flags);
  if (st != pc::JOB) return no_slot(st, flags);
  const pc::Cluster c = L.clusters[k];
  if (!pc::cluster_ok(L, c)) return no_slot(pc::BROKEN, pc::FLAG_BOUNDS);
  const int32_t m0 = L.members[(size_t)c.member_begin];
  if (m0 < 0 || m0 >= fr.match_count) return no_slot(pc::BROKEN, pc::FLAG_BOUNDS);
  const int32_t first_class = L.matches[(size_t)fr.match_begin + (size_t)m0].class_index;
  const Scan s = scan(fr, c, first_class);
  if (s.bad_member || s.mixed) return no_slot(pc::BROKEN, pc::FLAG_BOUNDS);
  if (class_index >= 0 && first_class != class_index) return no_slot(pc::NO_JOB_CLASS, 0u);
  if (s.bad_view) return no_slot(pc::NO_JOB_BOUNDS, pc::FLAG_BOUNDS);
  return Slot{pc::JOB, 0u, fr.frame, fr.match_begin, fr.match_count, c.member_begin, c.member_count};
}

// ---- the winner and the record ----------------------------------------------------------------------------------------------------------------
// idx: scratch of n entries.
LMX_RP_FN int32_t winning_group(const int32_t* size, int32_t n, int32_t* idx) {
  for (int32_t g = 0; g < n; ++g) idx[g] = g;
  sortemu::sort(idx, n, [&](int32_t i, int32_t j) { return size[i] > size[j]; });
  return idx[0];
}

struct Sums { double q[4], distance, D, ori_dist; int64_t x, y; int32_t count, hole; };

LMX_RP_FN void sums_init(Sums* s) {
  s->q[0] = s->q[1] = s->q[2] = s->q[3] = 0.0; s->distance = s->D = s->ori_dist = 0.0;
  s->x = s->y = 0; s->count = 0; s->hole = 0;
}

LMX_RP_FN void sums_add(Sums* s, const double* q, double distance, double D, double ori_dist, int32_t x, int32_t y) {
  for (int k = 0; k < 4; ++k) s->q[k] = s->q[k] + q[k];
  s->distance = s->distance + distance; s->D = s->D + D; s->ori_dist = s->ori_dist + ori_dist;
  s->x += x; s->y += y; s->count += 1;
  const double d = D - ori_dist;
  if ((d < 0.0 ? -d : d) < 0.001) s->hole = 1;
}

LMX_RP_FN void record_zero(Record* r) {
  for (int k = 0; k < 9; ++k) r->R[k] = 0.0;
  r->distance = r->D = r->ori_dist = 0.0;
  r->x = r->y = r->n_members = r->n_groups = r->group = r->n_group_members = r->front = r->center_hole = 0;
  r->rect[0] = r->rect[1] = r->rect[2] = r->rect[3] = 0;
  r->n_model = 0; r->status = NONE;
}

LMX_RP_FN void record_too_many(int32_t n_members, Record* r) {
  record_zero(r);
  r->n_members = n_members; r->n_groups = kMaxGroups; r->status = TOO_MANY_GROUPS;
}

// The record of a slot whose groups are made.  false: the mean position is out of range (NO_JOB_BOUNDS: the caller zeroes the record).
LMX_RP_FN bool record_of_sums(const Sums& s, int32_t n_members, int32_t n_groups, int32_t group, int32_t front, Record* r) {
  record_zero(r);
  const int64_t n = s.count;
  const int64_t mx = s.x / n, my = s.y / n;
  if (mx < -(int64_t)kMaxMean || mx > (int64_t)kMaxMean || my < -(int64_t)kMaxMean || my > (int64_t)kMaxMean) return false;
  const double dn = (double)s.count;
  r->distance = s.distance / dn; r->D = s.D / dn; r->ori_dist = s.ori_dist / dn;
  r->x = (int32_t)mx; r->y = (int32_t)my;
  r->n_members = n_members; r->n_groups = n_groups; r->group = group; r->n_group_members = s.count; r->front = front; r->center_hole = s.hole;
  const double x = s.q[0] / dn, y = s.q[1] / dn, z = s.q[2] / dn, w = s.q[3] / dn;
  const double n2 = ((x * x + y * y) + z * z) + w * w;
  if (!(n2 > 0.0) || !(n2 <= 1.7976931348623157e308)) { r->status = DEGENERATE; return true; }
  const double len = sqrt(n2);
  rot_of_quat(x / len, y / len, z / len, w / len, r->R);
  r->status = OK;
  return true;
}

// ---- the whole decision on one thread (CPU builds) -----------------------------------------------------------------------------------------
// member_group: parallel to L.members, written for a JOB slot's members only.  -> the slot; *rec its record.
LMX_RP_FN Slot resolve_slot(const pc::Lists& L, const View* views, int32_t n_views, double trace_min, int32_t class_index, uint32_t k, int32_t* member_group,
                            Record* rec, int n_lanes = pc::kLanes) {
  record_zero(rec);
  int32_t claims = 0, first = INT32_MAX;
  for (int32_t f = 0; f < L.n_frames; ++f)
    if (pc::frame_claims(L, f, k)) { claims += 1; first = f < first ? f : first; }
  Slot s = slot_from_claims(L, class_index, k, claims, first, [&](const pc::Frame& fr, const pc::Cluster& c, int32_t first_class) {
    Scan all = {0, 0, 0};
    for (int l = 0; l < n_lanes; ++l) {
      const Scan one = scan_of_lane(L, fr, c, n_views, first_class, l, n_lanes);
      all.bad_member |= one.bad_member; all.bad_view |= one.bad_view; all.mixed |= one.mixed;
    }
    return all;
  });
  if (s.state != pc::JOB) return s;
  static_assert(kMaxGroups <= 512, "the arrays below");
  int32_t size[kMaxGroups], front[kMaxGroups], idx[kMaxGroups];
  double fR[kMaxGroups][9];
  int32_t n_groups = 0;
  auto match_of = [&](int32_t p) { return s.match_begin + L.members[(size_t)s.member_begin + (size_t)p]; };
  for (int32_t p = 0; p < s.member_count; ++p) {
    const double* Rp = views[L.matches[match_of(p)].template_id].R;
    int32_t g = 0;
    while (g < n_groups && !(trace_dot(Rp, fR[g]) > trace_min)) ++g;
    if (g == n_groups) {
      if (n_groups == kMaxGroups) {
        for (int32_t q = p; q < s.member_count; ++q) member_group[(size_t)s.member_begin + (size_t)q] = -1;
        record_too_many(s.member_count, rec);
        return s;
      }
      for (int k9 = 0; k9 < 9; ++k9) fR[g][k9] = Rp[k9];
      size[g] = 0; front[g] = match_of(p);
      n_groups += 1;
    }
    size[g] += 1;
    member_group[(size_t)s.member_begin + (size_t)p] = g;
  }
  const int32_t win = winning_group(size, n_groups, idx);
  Sums sums;
  sums_init(&sums);
  for (int32_t p = 0; p < s.member_count; ++p) {
    if (member_group[(size_t)s.member_begin + (size_t)p] != win) continue;
    const pc::Match& m = L.matches[match_of(p)];
    const View& v = views[m.template_id];
    sums_add(&sums, v.q, v.distance, v.D, v.ori_dist, m.x, m.y);
  }
  if (!record_of_sums(sums, s.member_count, n_groups, win, front[win], rec)) {
    record_zero(rec);
    s = no_slot(pc::NO_JOB_BOUNDS, pc::FLAG_BOUNDS);
  }
  return s;
}

}  // namespace rp
}  // namespace lmx
