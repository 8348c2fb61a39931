// Pose refinement of a match against the scene depth (lmx_pose_refine_matches, include/lmx.h): the arithmetic of one pixel, one pass, one
// solve and one job, shared by the HIP kernel (lmx_verify.hip, k_pose_refine) and -- compiled with LMX_PR_HOST -- by plain CPU builds
// (tests/cpp/pose_refine_host.cpp).  The stage stands where the reference runs icpPoseRefine (src/rgbdDetector.cpp:1263-1412, PCL's
// point-to-point ICP); PCL is not part of the reference, so the definition below is this repository's own.  It uses + - * / sqrt rint
// llrint on doubles and 64-bit integer sums and nothing else, every expression in the written order (build with -ffp-contract=off), so
// that the CPU build and gfx950 agree bit for bit.  This comment is the specification; tests/pose_refine_cases.py restates it in numpy.
//
// UNITS  millimetres in double precision; "ticks" are 1/16 mm as int64.  llrint / rint round to nearest, ties to even.
//
// INPUT  a template crop t[h][w] (uint16 mm, 0 = not on the object) whose pixel (0, 0) was rendered at pixel (rect_x, rect_y) of the model
//   camera (fx_m, fy_m, cx_m, cy_m); a scene depth image s[H][W] (uint16 mm, 0 = no measurement) of the scene camera (fx_s, ..); a match
//   at (x, y); the parameters max_dist_mm, eps_rot_rad, eps_trans_mm, max_iterations (0..64), min_pairs (>= 3), search_radius (0..2).
//
// POINTS  back(cam, a, b, d) = ( (((double)a - cx) * (double)d) * ifx,  (((double)b - cy) * (double)d) * ify,  (double)d ) with the
//   reciprocals ifx = 1 / fx, ify = 1 / fy, each one division (a product with them costs the device a tenth of a division, and a pass
//   takes one such point per candidate).
//   Model point of crop pixel (i, j) with t = crop[i][j] != 0:  u = rect_x + j, v = rect_y + i, M = back(model, u, v, t).
//   Scene point of pixel (X, Y) with s = scene[Y][X] != 0:      Q = back(scene, X, Y, s).      n_model = #{t != 0}.
//
// STEP 0, PLACEMENT  The pairs are those of the depth term (lmx_depth_verify.hpp): crop pixel (i, j) meets scene pixel (X, Y) =
//   (x + j, y + i) under dv::scene_col / dv::scene_row; it pairs iff t != 0, (X, Y) lies inside the image and s != 0.  Over the pairs, as
//   int64:  n0, St = sum t, Sut = sum u t, Svt = sum v t, Ss = sum s, SXs = sum X s, SYs = sum Y s.   n0 < min_pairs: status NO_OVERLAP,
//   R = I, t = 0, nothing else runs.  Otherwise, with N = (double)n0:
//     m0 = ( (((double)Sut - cx_m * (double)St) / fx_m) / N,  (((double)Svt - cy_m * (double)St) / fy_m) / N,  (double)St / N )
//     q0 = the same expression of SXs, SYs, Ss and the scene camera;      quaternion (w, x, y, z) = (1, 0, 0, 0), R_0 = I, t_0 = q0 - m0.
//
// PASS k (association under the pose R, t)   c = R m0 + t, every row ((R[0] m0.x + R[1] m0.y) + R[2] m0.z) + t.x;  C = llrint(16 c).
//   dmax = llrint(16 max_dist_mm).  For every model pixel (t != 0), with the same row expression:
//     p = R M + t.   Skip the pixel unless p.z >= 1 and |p.x|, |p.y|, |p.z| <= 2^20.
//     xr = rint((p.x * fx_s) / p.z + cx_s), yr likewise.  Skip unless |xr|, |yr| <= 2^20.  X0 = (int)xr, Y0 = (int)yr.
//     P = llrint(16 p).  Candidates: scene pixels (X0 + dx, Y0 + dy), |dx|, |dy| <= search_radius, dy outer, dx inner (raster order),
//     inside the image, s != 0, |Q.x|, |Q.y| <= 2^21 (farther than any pair's partner: P lies within 2^20, dmax within 2^10 mm; it keeps
//     16 Q, like 16 p, inside int32).  For a candidate D = llrint(16 Q) - P; it is admissible iff |D.x|, |D.y|, |D.z| <= dmax (which every
//     candidate with |D|^2 <= dmax^2 is; it keeps |D|^2 inside int64).  The pair is the admissible candidate of smallest integer
//     |D|^2, the first one on a tie; it is accepted iff |D|^2 <= dmax^2.
//     P' = P - C.  The pair is dropped if |P'.x|, |P'.y| or |P'.z| > 2^15.
//   The 17 sums of a pass, int64, independent of the order of summation:
//     [0] n   [1..3] sum P'   [4..6] sum D   [7..12] sum of P'x P'x, P'x P'y, P'x P'z, P'y P'y, P'y P'z, P'z P'z
//     [13..15] sum P' x D = (P'y Dz - P'z Dy, P'z Dx - P'x Dz, P'x Dy - P'y Dx)   [16] sum |D|^2
//   Bounds (static_asserted below): |P'| <= 2^15, |D| <= dmax <= 2^14 (max_dist_mm <= 1024) and at most 2^28 pixels in a crop keep every
//   sum below 2^63; the placement sums need |u|, |v|, X, Y < 2^18, which the host checks (frame sides and rect corners).
//   rms of a pass = n > 0 ? sqrt((double)[16] / (double)n) / 16 : 0.
//
// SOLVE  minimise sum |w x P' + v - D|^2 over the rotation vector w (radians) and the translation v (ticks):
//     A (w, v) = b,   A = [[S, [sum P']x], [[sum P']x^T, n I]],  S = sum(|P'|^2 I - P' P'^T),   b = (sum P' x D, sum D)
//   with [a]x = [[0, -az, ay], [az, 0, -ax], [-ay, ax, 0]].  S's entries are formed as int64 (S00 = [10] + [12], S01 = -[8], ..), then every
//   entry of A and b is converted to double.  Cholesky A = L L^T, column j = 0..5:  d = A[j][j]; for k < j: d = d - L[j][k] L[j][k];
//   the pivot d must be > 0; L[j][j] = sqrt(d); for i > j: e = A[i][j]; for k < j: e = e - L[i][k] L[j][k]; L[i][j] = e / L[j][j].
//   Forward  y[i] = (b[i] - sum_{k<i, ascending} L[i][k] y[k]) / L[i][i];  back, i = 5..0:  z[i] = (y[i] - sum_{k>i, ascending} L[k][i] z[k]) / L[i][i],
//   each sum subtracted term by term.  w = z[0..2], v = z[3..5].  The full step is taken iff every pivot was > 0, w.w <= 1 and
//   v.v <= 2^48 (comparisons that a NaN fails); otherwise the step is translation-only: w = 0, v = sum D / (double)n.
//
// UPDATE  h = w / 2;  g = sqrt(((1 + h.x h.x) + h.y h.y) + h.z h.z);  dq = (1 / g, h.x / g, h.y / g, h.z / g).
//   q' = dq (x) q, the Hamilton product, each component summed left to right:
//     w' = dw qw - dx qx - dy qy - dz qz      x' = dw qx + dx qw + dy qz - dz qy
//     y' = dw qy - dx qz + dy qw + dz qx      z' = dw qz + dx qy - dy qx + dz qw
//   then q' / sqrt(((w'w' + x'x') + y'y') + z'z').   R(q) = [[1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy)], [2 (xy + wz), 1 - 2 (xx + zz), 2 (yz - wx)],
//   [2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)]].  dR = R(dq), R_{k+1} = R(q'), and with e = t - c:
//     t_{k+1} = (c + dR e) + v / 16,  row-wise (c.x + ((dR[0] e.x + dR[1] e.y) + dR[2] e.z)) + v.x / 16.
//   The step has CONVERGED iff sqrt((w.x w.x + w.y w.y) + w.z w.z) <= eps_rot_rad and sqrt((v.x v.x + v.y v.y) + v.z v.z) / 16 <= eps_trans_mm.
//
// CONTROL  status = MAX_ITERATIONS, final = (max_iterations == 0).  For k = 0, 1, ..: run pass k under the current pose.
//   k == 0: n_pairs_first = n, rms_first_mm = rms.   If final: n_pairs_last = n, rms_last_mm = rms, stop.
//   n < min_pairs: status LOST, n_pairs_last = n, rms_last_mm = rms, the pose stays, stop.
//   Solve, update, iterations = k + 1.  Converged: status CONVERGED, final.  Else k + 1 == max_iterations: final.
//   So iterations + 1 passes run, the last one only fills n_pairs_last / rms_last_mm (unless LOST), and the record carries the last pose.
//
// SCHEDULE (refine_job_staged; lmx_depth_templates_set_refine_schedule)  1 to 4 stages where the above has one; the reference's icpPoseRefine
//   runs a coarse and a fine alignment fed into one another (src/rgbdDetector.cpp:1314-1367) over a thinned model cloud (:1294-1295).  A stage
//   has its own max_dist_mm, eps_rot_rad, eps_trans_mm, max_iterations, search_radius, each in the range above, and a stride in {1, 2, 4, 8};
//   a stage that is not the last has max_iterations >= 1.  The cameras and min_pairs are those of the parameters, for every stage.
//   STEP 0 is unchanged: every crop pixel takes part, n_model counts every pixel, m0 is the one centroid of all stages.
//   The selected pixels of a stage are the crop pixels with t != 0, i % stride == 0 and j % stride == 0 (i, j crop-local: the rect plays
//   no part; the crop of a rough pose, lmx_rough_pose_chain_on, is the silhouette box of its render, lmx_rough_pose_t's rect).  A pass of the stage is PASS k over the selected pixels alone, under the stage's dmax and search_radius; a selected pixel's
//   arithmetic is unchanged.
//   Control: stage 0 starts from the placement's pose, q included; inside a stage the passes count from k = 0 and the stage starts with
//   status = MAX_ITERATIONS.  The first pass of stage 0 fills n_pairs_first / rms_first_mm.  n < min_pairs in any pass that would solve:
//   status LOST, n_pairs_last = n, rms_last_mm = rms, the pose stays, everything stops.  A stage that is not the last: solve, update with the
//   stage's eps, iterations += 1; converged: status CONVERGED; converged or k + 1 == max_iterations: the stage ends -- it runs no measuring
//   pass, and pass 0 of the next stage runs under exactly the q, R, t it left.  The last stage is CONTROL with the stage's parameters, its
//   measuring pass included.  iterations is the total over the stages, status that of the last stage that ran, reserved the index of the
//   stage in which the record was finished (0 for NO_OVERLAP).  One stage of stride 1 is refine_job in every byte.
//   The debug sums are [sum of max_iterations + 1][17], one row per pass in the order the passes ran.
//
// PLANE (refine_job_plane; lmx_depth_templates_set_refine_plane)  A stage has a point_shift.  With -1 it is the stage above in every byte.  With
//   k in 0..20 the stage minimises the point-to-plane distance against the scene's stored normals (lmx_normal_verify.hpp, nv::Packed: the
//   normal map of the job's frame, one element per scene pixel), held in place by the point-to-point term weighted 2^-k.
//   Pass: PASS k is unchanged, its 17 sums included.  For every pair that enters the 17 sums let N = (Nx, Ny, Nz) be the stored normal at the
//   scene pixel of the chosen candidate (inside the image by construction; one 8-byte load after the selection).  If N is valid, with int64
//   and rs14(a) = (a + 8192) >> 14, an arithmetic shift:
//     c = (rs14(P'y Nz - P'z Ny), rs14(P'z Nx - P'x Nz), rs14(P'x Ny - P'y Nx)),  r = rs14(D.x Nx + D.y Ny + D.z Nz),  g = (c.x, c.y, c.z, Nx, Ny, Nz)
//   The 29 plane sums:  [0] n_plane   [1..21] sum g_i g_j for i <= j, row-major (00, 01, .., 05, 11, .., 55)   [22..27] sum g_i r   [28] sum r^2
//   Bounds (static_asserted below): |P'| <= 2^15, |N| <= 2^14 and |D| <= 2^14 give |c|, |r| < 2^17, every product is below 2^34, and 2^28
//   pixels keep every sum below 2^63.
//   Step: n_plane < min_pairs: (w, v) is SOLVE's, bit for bit.  Otherwise, with SOLVE's integer matrix Ai and its right side b_pt:
//     lambda = 1.0 / (double)(1 << k);   s_i = 1 for i < 3, 1.0 / 16384.0 for i >= 3
//     G[i][j] = ((double)sum_ij * s_i) * s_j      h[i] = (double)sum_ir * s_i
//     A[i][j] = G[i][j] + lambda * (double)Ai[i][j]      b[i] = h[i] + lambda * b_pt[i]
//   then SOLVE's Cholesky, substitutions and acceptance test (every pivot > 0, w.w <= 1, v.v <= 2^48) on A, b; if any of them fails the step
//   is SOLVE's, its translation-only fallback included.  w is in radians and v in ticks as in SOLVE: minimise sum (N . (w x P' + v - D))^2
//   + lambda sum |w x P' + v - D|^2 with N a unit vector.  UPDATE, CONTROL and SCHEDULE are unchanged; rms_* stay the point-to-point
//   distances, n < min_pairs still means LOST.
//   Why the point term: on a flat patch all normals are parallel and the plane system alone has rank 3; the lambda-weighted point term keeps
//   it positive definite wherever SOLVE's own system is.  The normal is this repository's own (deviations): it neglects the
//   off-axis perspective terms; on consistent data the fixed point of the metric does not depend on the normals.
//   The debug plane sums are [sum of max_iterations + 1][29], row for row next to the 17; the rows of passes of a -1 stage are left alone.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef LMX_PR_HOST
#ifndef LMX_DV_HOST
#define LMX_DV_HOST
#endif
#ifndef LMX_NV_HOST
#define LMX_NV_HOST
#endif
#define LMX_PR_FN inline
#else
#define LMX_PR_FN __host__ __device__ __forceinline__
#endif

#include "lmx_depth_verify.hpp"
#include "lmx_normal_verify.hpp"

namespace lmx {
namespace pr {

constexpr int kSums = 17;
constexpr int kPlaceSums = 8;            // n0, St, Sut, Svt, Ss, SXs, SYs, n_model
constexpr int kMaxIterations = 64;
constexpr int kMaxSearchRadius = 2;
constexpr double kMaxDistMm = 1024.0;
constexpr int64_t kMaxCentredTicks = (int64_t)1 << 15;
constexpr int64_t kMaxCoord = (int64_t)1 << 18;   // |u|, |v|, X, Y stay below it
constexpr double kMaxPointMm = 1048576.0;         // 2^20
constexpr double kMaxStepTicksSq = 281474976710656.0;   // 2^48
// the largest term of each kind times the most pixels a crop holds (dv::kMaxCropSide^2 = 2^28) stays below 2^63
constexpr int64_t kMaxPixels = (int64_t)dv::kMaxCropSide * dv::kMaxCropSide;
constexpr int64_t kMaxDTicks = (int64_t)(16 * 1024);
static_assert(kMaxPixels == ((int64_t)1 << 28), "a crop holds at most 2^28 pixels");
static_assert(kMaxCentredTicks * kMaxCentredTicks <= (INT64_MAX / kMaxPixels), "sum P' P'^T fits int64");
static_assert(2 * kMaxCentredTicks * kMaxDTicks <= (INT64_MAX / kMaxPixels), "sum P' x D fits int64");
static_assert(3 * kMaxDTicks * kMaxDTicks <= (INT64_MAX / kMaxPixels), "sum |D|^2 fits int64");
static_assert(kMaxCoord * 65535 <= (INT64_MAX / kMaxPixels), "the placement sums fit int64");

// PLANE: the 29 sums, the shifts, the bounds of their terms
constexpr int kPlaneSums = 29;
constexpr int kAllSums = kSums + kPlaneSums;   // what a lane of a plane pass accumulates
constexpr int kMaxPointShift = 20;
constexpr int64_t kMaxNormal = (int64_t)nv::kUnit;                                        // |N| <= 2^14
constexpr int64_t kMaxPlaneTerm = (int64_t)1 << 17;                                       // |c|, |r| stay below it
static_assert(kMaxNormal == ((int64_t)1 << 14), "a stored normal's components lie within 2^14");
static_assert(((2 * kMaxCentredTicks * kMaxNormal + 8192) >> 14) < kMaxPlaneTerm, "|c| < 2^17");
static_assert(((3 * kMaxDTicks * kMaxNormal + 8192) >> 14) < kMaxPlaneTerm, "|r| < 2^17");
static_assert(kMaxPlaneTerm * kMaxPlaneTerm <= (INT64_MAX / kMaxPixels), "the plane sums fit int64");
static_assert(((int64_t)-1 >> 14) == -1 && (((int64_t)-8193 + 8192) >> 14) == -1 && (((int64_t)-24577 + 8192) >> 14) == -2 && (((int64_t)24575 + 8192) >> 14) == 1,
              "rs14: >> of a negative int64 is an arithmetic shift");

enum Status : int32_t { NONE = 0, CONVERGED = 1, MAX_ITERATIONS = 2, NO_OVERLAP = 3, LOST = 4 };

struct Camera { double fx, fy, cx, cy; };
struct Inverse { double fx, fy; };   // 1 / fx, 1 / fy of a camera
struct Params {
  Camera model, scene;
  double max_dist_mm, eps_rot_rad, eps_trans_mm;
  int32_t max_iterations, min_pairs, search_radius, pad;
};
struct Pose { double q[4], R[9], t[3]; };
struct Record {   // the bytes of lmx_pose_refine_t
  double R[9], t_mm[3];
  double rms_first_mm, rms_last_mm;
  int32_t n_model, n_pairs_first, n_pairs_last, iterations, status, reserved;
};
struct Control { int32_t final_pass; };
constexpr int kMaxStages = 4;
struct Stage {   // the bytes of lmx_pose_refine_stage
  double max_dist_mm, eps_rot_rad, eps_trans_mm;
  int32_t max_iterations, search_radius, stride, pad;
};
struct Schedule { int32_t n_stages, pad; Stage stage[kMaxStages]; };
struct StagedControl { int32_t stage, k, final_pass; };   // the stage, the pass inside it, "this pass only measures"
struct PlaneShifts { int32_t shift[kMaxStages]; };          // a stage's point_shift: -1 the point-to-point stage, 0..20 PLANE
constexpr PlaneShifts kNoPlane = {{-1, -1, -1, -1}};
LMX_PR_FN bool any_plane(const PlaneShifts& K, int32_t n_stages) {
  bool any = false;
  for (int32_t k = 0; k < n_stages && k < kMaxStages; ++k) any = any || K.shift[k] >= 0;
  return any;
}

LMX_PR_FN Inverse inverse_of(const Camera& cam) { return Inverse{1.0 / cam.fx, 1.0 / cam.fy}; }

LMX_PR_FN void back(const Camera& cam, const Inverse& inv, int64_t a, int64_t b, uint16_t d, double out[3]) {
  const double z = (double)d;
  out[0] = (((double)a - cam.cx) * z) * inv.fx;
  out[1] = (((double)b - cam.cy) * z) * inv.fy;
  out[2] = z;
}

// llrint(16 a) for |a| <= 2^21 mm: the product fits an int32, which the device converts to in one instruction (it has none for int64)
LMX_PR_FN int64_t ticks_of(double a) { return (int64_t)(int32_t)rint(16.0 * a); }
constexpr double kMaxScenePointMm = 2097152.0;   // 2^21

LMX_PR_FN void mat_point(const double R[9], const double a[3], const double t[3], double out[3]) {
  out[0] = ((R[0] * a[0] + R[1] * a[1]) + R[2] * a[2]) + t[0];
  out[1] = ((R[3] * a[0] + R[4] * a[1]) + R[5] * a[2]) + t[1];
  out[2] = ((R[6] * a[0] + R[7] * a[1]) + R[8] * a[2]) + t[2];
}

LMX_PR_FN void rotation_of(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// ---- step 0 ---------------------------------------------------------------------------------------------------------------------------
// One crop pixel t != 0 at (i, j); (X, Y, s): the scene pixel it meets, s == 0 when it meets none (outside the image, or no measurement).
LMX_PR_FN void place_pixel(int32_t rect_x, int32_t rect_y, int32_t i, int32_t j, uint16_t t, int32_t X, int32_t Y, uint16_t s, int64_t a[kPlaceSums]) {
  a[7] += 1;
  if (s == 0) return;
  const int64_t u = (int64_t)rect_x + j, v = (int64_t)rect_y + i;
  a[0] += 1; a[1] += t; a[2] += u * t; a[3] += v * t;
  a[4] += s; a[5] += (int64_t)X * s; a[6] += (int64_t)Y * s;
}

LMX_PR_FN void centroid_of(const Camera& cam, int64_t n, int64_t sd, int64_t sad, int64_t sbd, double out[3]) {
  const double N = (double)n;
  out[0] = (((double)sad - cam.cx * (double)sd) / cam.fx) / N;
  out[1] = (((double)sbd - cam.cy * (double)sd) / cam.fy) / N;
  out[2] = (double)sd / N;
}

// The record's start and, with enough pairs, the start pose.  False: NO_OVERLAP, the record is final.
LMX_PR_FN bool placement(const Params& P, const int64_t a[kPlaceSums], double m0[3], Pose* pose, Record* r, Control* ctl) {
  for (int k = 0; k < 9; ++k) r->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  r->t_mm[0] = r->t_mm[1] = r->t_mm[2] = 0.0;
  r->rms_first_mm = r->rms_last_mm = 0.0;
  r->n_model = (int32_t)a[7];
  r->n_pairs_first = r->n_pairs_last = r->iterations = r->reserved = 0;
  r->status = NO_OVERLAP;
  if (a[0] < (int64_t)P.min_pairs) return false;
  double q0[3];
  centroid_of(P.model, a[0], a[1], a[2], a[3], m0);
  centroid_of(P.scene, a[0], a[4], a[5], a[6], q0);
  pose->q[0] = 1.0; pose->q[1] = pose->q[2] = pose->q[3] = 0.0;
  rotation_of(pose->q, pose->R);
  for (int k = 0; k < 3; ++k) pose->t[k] = q0[k] - m0[k];
  r->status = MAX_ITERATIONS;
  ctl->final_pass = P.max_iterations == 0;
  return true;
}

// ---- a pass ---------------------------------------------------------------------------------------------------------------------------
LMX_PR_FN void centre_of(const Pose& pose, const double m0[3], double c[3], int64_t C[3]) {
  mat_point(pose.R, m0, pose.t, c);
  for (int k = 0; k < 3; ++k) C[k] = (int64_t)llrint(16.0 * c[k]);
}

LMX_PR_FN int64_t dist_ticks(double max_dist_mm) { return (int64_t)llrint(16.0 * max_dist_mm); }
LMX_PR_FN int64_t max_dist_ticks(const Params& P) { return dist_ticks(P.max_dist_mm); }

LMX_PR_FN bool within(double a, double bound) { return a >= -bound && a <= bound; }   // false for a NaN

// PLANE: the 29 terms of a pair (x, y, z) = P', D with the valid stored normal N.
LMX_PR_FN int64_t rs14(int64_t a) { return (a + 8192) >> 14; }

LMX_PR_FN void plane_terms(int64_t x, int64_t y, int64_t z, const int64_t D[3], nv::Packed N, int64_t pl[kPlaneSums]) {
  const int64_t nx = nv::comp(N, 0), ny = nv::comp(N, 1), nz = nv::comp(N, 2);
  const int64_t g[6] = {rs14(y * nz - z * ny), rs14(z * nx - x * nz), rs14(x * ny - y * nx), nx, ny, nz};
  const int64_t r = rs14(D[0] * nx + D[1] * ny + D[2] * nz);
  pl[0] += 1;
  int q = 1;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) pl[q++] += g[i] * g[j];
  for (int i = 0; i < 6; ++i) pl[22 + i] += g[i] * r;
  pl[28] += r * r;
}

// One model pixel (t != 0) of crop pixel (i, j) under `pose`.  frame: the scene, H rows of scene_pitch elements, read only inside the image.
// RAD: the search radius as a constant, so that the window unrolls: its scene values are all loaded first (independent loads, one wait),
// then the candidates are taken in raster order.
// PLANE: the pair's 29 terms as well (pl), with the normal read at the chosen candidate's pixel of `normals` (the frame's normal map, rows
// of scene_pitch elements like the frame's); without it neither is touched and the code is that of the 17 sums alone.
template <int RAD, bool PLANE>
LMX_PR_FN void pass_pixel_core(const Params& P, const Inverse& im, const Inverse& is, const Pose& pose, const int64_t C[3], int64_t dmax, int32_t rect_x, int32_t rect_y, int32_t i,
                               int32_t j, uint16_t t, const uint16_t* frame, const nv::Packed* normals, int32_t W, int32_t H, size_t scene_pitch, int64_t a[kSums],
                               int64_t* pl) {
  double M[3], p[3];
  back(P.model, im, (int64_t)rect_x + j, (int64_t)rect_y + i, t, M);
  mat_point(pose.R, M, pose.t, p);
  if (!(p[2] >= 1.0) || !within(p[0], kMaxPointMm) || !within(p[1], kMaxPointMm) || !within(p[2], kMaxPointMm)) return;
  const double xr = rint((p[0] * P.scene.fx) / p[2] + P.scene.cx), yr = rint((p[1] * P.scene.fy) / p[2] + P.scene.cy);
  if (!within(xr, kMaxPointMm) || !within(yr, kMaxPointMm)) return;
  const int32_t X0 = (int32_t)xr, Y0 = (int32_t)yr;
  int64_t Pt[3];
  for (int k = 0; k < 3; ++k) Pt[k] = ticks_of(p[k]);
  constexpr int SIDE = 2 * RAD + 1;
  uint16_t sv[SIDE * SIDE];
#ifndef LMX_PR_HOST
#pragma unroll
#endif
  for (int q = 0; q < SIDE * SIDE; ++q) {
    const int32_t X = X0 + (q % SIDE - RAD), Y = Y0 + (q / SIDE - RAD);
    const bool in = X >= 0 && X < W && Y >= 0 && Y < H;
    sv[q] = in ? frame[(size_t)(in ? Y : 0) * scene_pitch + (size_t)(in ? X : 0)] : (uint16_t)0;   // the only scene read, inside the image
  }
  bool found = false;
  int64_t best = 0, D[3] = {0, 0, 0};
  int bq = 0;   // PLANE: the chosen candidate's place in the window
#ifndef LMX_PR_HOST
#pragma unroll
#endif
  for (int q = 0; q < SIDE * SIDE; ++q) {
    const uint16_t s = sv[q];
    if (s == 0) continue;   // outside the image, or no measurement
    double Q[3];
    back(P.scene, is, (int64_t)X0 + (q % SIDE - RAD), (int64_t)Y0 + (q / SIDE - RAD), s, Q);
    if (!within(Q[0], kMaxScenePointMm) || !within(Q[1], kMaxScenePointMm)) continue;
    int64_t d[3];
    for (int k = 0; k < 3; ++k) d[k] = ticks_of(Q[k]) - Pt[k];
    if (d[0] < -dmax || d[0] > dmax || d[1] < -dmax || d[1] > dmax || d[2] < -dmax || d[2] > dmax) continue;
    const int64_t dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!found || dd < best) { found = true; best = dd; D[0] = d[0]; D[1] = d[1]; D[2] = d[2]; if (PLANE) bq = q; }
  }
  if (!found || best > dmax * dmax) return;
  const int64_t x = Pt[0] - C[0], y = Pt[1] - C[1], z = Pt[2] - C[2];
  if (x < -kMaxCentredTicks || x > kMaxCentredTicks || y < -kMaxCentredTicks || y > kMaxCentredTicks || z < -kMaxCentredTicks || z > kMaxCentredTicks) return;
  a[0] += 1;
  a[1] += x; a[2] += y; a[3] += z;
  a[4] += D[0]; a[5] += D[1]; a[6] += D[2];
  a[7] += x * x; a[8] += x * y; a[9] += x * z; a[10] += y * y; a[11] += y * z; a[12] += z * z;
  a[13] += y * D[2] - z * D[1]; a[14] += z * D[0] - x * D[2]; a[15] += x * D[1] - y * D[0];
  a[16] += best;
  if (PLANE) {
    const int32_t X = X0 + (bq % SIDE - RAD), Y = Y0 + (bq / SIDE - RAD);   // a candidate's pixel: inside the image
    const nv::Packed N = normals[(size_t)Y * scene_pitch + (size_t)X];
    if (nv::valid(N)) plane_terms(x, y, z, D, N, pl);
  }
}

template <int RAD>
LMX_PR_FN void pass_pixel_r(const Params& P, const Inverse& im, const Inverse& is, const Pose& pose, const int64_t C[3], int64_t dmax, int32_t rect_x, int32_t rect_y, int32_t i, int32_t j,
                            uint16_t t, const uint16_t* frame, int32_t W, int32_t H, size_t scene_pitch, int64_t a[kSums]) {
  pass_pixel_core<RAD, false>(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, nullptr, W, H, scene_pitch, a, nullptr);
}

// radius: the search radius in force (a stage's, or the parameters'); of P the cameras alone are read.
LMX_PR_FN void pass_pixel_rad(const Params& P, int32_t radius, const Inverse& im, const Inverse& is, const Pose& pose, const int64_t C[3], int64_t dmax, int32_t rect_x, int32_t rect_y,
                              int32_t i, int32_t j, uint16_t t, const uint16_t* frame, int32_t W, int32_t H, size_t scene_pitch, int64_t a[kSums]) {
  switch (radius) {
    case 0: pass_pixel_r<0>(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, W, H, scene_pitch, a); break;
    case 1: pass_pixel_r<1>(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, W, H, scene_pitch, a); break;
    default: pass_pixel_r<2>(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, W, H, scene_pitch, a); break;
  }
}

// The plane form of a pass pixel: pass_pixel_rad's 17 sums into a, the pair's 29 plane sums into pl.
LMX_PR_FN void pass_pixel_plane_rad(const Params& P, int32_t radius, const Inverse& im, const Inverse& is, const Pose& pose, const int64_t C[3], int64_t dmax, int32_t rect_x,
                                    int32_t rect_y, int32_t i, int32_t j, uint16_t t, const uint16_t* frame, const nv::Packed* normals, int32_t W, int32_t H, size_t scene_pitch,
                                    int64_t a[kSums], int64_t pl[kPlaneSums]) {
  switch (radius) {
    case 0: pass_pixel_core<0, true>(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, normals, W, H, scene_pitch, a, pl); break;
    case 1: pass_pixel_core<1, true>(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, normals, W, H, scene_pitch, a, pl); break;
    default: pass_pixel_core<2, true>(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, normals, W, H, scene_pitch, a, pl); break;
  }
}

LMX_PR_FN void pass_pixel(const Params& P, const Inverse& im, const Inverse& is, const Pose& pose, const int64_t C[3], int64_t dmax, int32_t rect_x, int32_t rect_y, int32_t i, int32_t j,
                          uint16_t t, const uint16_t* frame, int32_t W, int32_t H, size_t scene_pitch, int64_t a[kSums]) {
  pass_pixel_rad(P, P.search_radius, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, frame, W, H, scene_pitch, a);
}

LMX_PR_FN double rms_of(const int64_t a[kSums]) { return a[0] > 0 ? sqrt((double)a[16] / (double)a[0]) / 16.0 : 0.0; }

// ---- solve and update -------------------------------------------------------------------------------------------------------------------
// The step (w, v) of a pass with n > 0.
LMX_PR_FN void solve(const int64_t a[kSums], double w[3], double v[3]) {
  const int64_t n = a[0], sx = a[1], sy = a[2], sz = a[3];
  const int64_t Ai[6][6] = {
      {a[10] + a[12], -a[8], -a[9], 0, -sz, sy},
      {-a[8], a[7] + a[12], -a[11], sz, 0, -sx},
      {-a[9], -a[11], a[7] + a[10], -sy, sx, 0},
      {0, sz, -sy, n, 0, 0},
      {-sz, 0, sx, 0, n, 0},
      {sy, -sx, 0, 0, 0, n}};
  const double b[6] = {(double)a[13], (double)a[14], (double)a[15], (double)a[4], (double)a[5], (double)a[6]};
  double L[6][6];
  bool ok = true;
  for (int j = 0; j < 6 && ok; ++j) {
    double d = (double)Ai[j][j];
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (!(d > 0.0)) { ok = false; break; }
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double e = (double)Ai[i][j];
      for (int k = 0; k < j; ++k) e = e - L[i][k] * L[j][k];
      L[i][j] = e / L[j][j];
    }
  }
  if (ok) {
    double y[6], z[6];
    for (int i = 0; i < 6; ++i) {
      double e = b[i];
      for (int k = 0; k < i; ++k) e = e - L[i][k] * y[k];
      y[i] = e / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
      double e = y[i];
      for (int k = i + 1; k < 6; ++k) e = e - L[k][i] * z[k];
      z[i] = e / L[i][i];
    }
    for (int k = 0; k < 3; ++k) { w[k] = z[k]; v[k] = z[3 + k]; }
    ok = ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) <= 1.0 && ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) <= kMaxStepTicksSq;
  }
  if (!ok) {
    const double N = (double)n;
    for (int k = 0; k < 3; ++k) { w[k] = 0.0; v[k] = (double)a[4 + k] / N; }
  }
}

// PLANE's step of a pass with n > 0: a the 17 sums, pl the 29, k the stage's point_shift (0..20).  One copy of the Cholesky serves the
// plane system and, where that is not taken, SOLVE's own (attempt 1: its matrix converted to double entry by entry, the same operations in
// the same order, so the same bits as solve()); it runs in place, L in A's lower triangle, so that the device's private arrays stay small.
LMX_PR_FN void solve_plane(const int64_t a[kSums], const int64_t pl[kPlaneSums], int32_t min_pairs, int32_t k, double w[3], double v[3]) {
  const int64_t n = a[0], sx = a[1], sy = a[2], sz = a[3];
  const double lambda = 1.0 / (double)((int64_t)1 << k);
  bool ok = false;
  for (int attempt = pl[0] >= (int64_t)min_pairs ? 0 : 1; attempt < 2 && !ok; ++attempt) {
    const int64_t Ai[6][6] = {
        {a[10] + a[12], -a[8], -a[9], 0, -sz, sy},
        {-a[8], a[7] + a[12], -a[11], sz, 0, -sx},
        {-a[9], -a[11], a[7] + a[10], -sy, sx, 0},
        {0, sz, -sy, n, 0, 0},
        {-sz, 0, sx, 0, n, 0},
        {sy, -sx, 0, 0, 0, n}};
    const double b_pt[6] = {(double)a[13], (double)a[14], (double)a[15], (double)a[4], (double)a[5], (double)a[6]};
    double A[6][6], b[6];   // the lower triangle of A alone is filled and read
    int q = 1;
#ifndef LMX_PR_HOST
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) {
      const double si = i < 3 ? 1.0 : 1.0 / 16384.0;
#ifndef LMX_PR_HOST
#pragma unroll
#endif
      for (int j = i; j < 6; ++j) {
        const double sj = j < 3 ? 1.0 : 1.0 / 16384.0;
        const double G = ((double)pl[q++] * si) * sj;
        A[j][i] = attempt == 0 ? G + lambda * (double)Ai[i][j] : (double)Ai[i][j];
      }
      b[i] = attempt == 0 ? (double)pl[22 + i] * si + lambda * b_pt[i] : b_pt[i];
    }
    ok = true;
    for (int j = 0; j < 6 && ok; ++j) {
      double d = A[j][j];
      for (int m = 0; m < j; ++m) d = d - A[j][m] * A[j][m];
      if (!(d > 0.0)) { ok = false; break; }
      A[j][j] = sqrt(d);
      for (int i = j + 1; i < 6; ++i) {
        double e = A[i][j];
        for (int m = 0; m < j; ++m) e = e - A[i][m] * A[j][m];
        A[i][j] = e / A[j][j];
      }
    }
    if (ok) {
      double y[6], z[6];
      for (int i = 0; i < 6; ++i) {
        double e = b[i];
        for (int m = 0; m < i; ++m) e = e - A[i][m] * y[m];
        y[i] = e / A[i][i];
      }
      for (int i = 5; i >= 0; --i) {
        double e = y[i];
        for (int m = i + 1; m < 6; ++m) e = e - A[m][i] * z[m];
        z[i] = e / A[i][i];
      }
      for (int m = 0; m < 3; ++m) { w[m] = z[m]; v[m] = z[3 + m]; }
      ok = ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) <= 1.0 && ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) <= kMaxStepTicksSq;
    }
  }
  if (!ok) {   // SOLVE's translation-only step
    const double N = (double)n;
    for (int m = 0; m < 3; ++m) { w[m] = 0.0; v[m] = (double)a[4 + m] / N; }
  }
}

// The pose after the step (w, v) about the centre c; true when the step is below both thresholds.
LMX_PR_FN bool update_eps(double eps_rot_rad, double eps_trans_mm, const double w[3], const double v[3], const double c[3], Pose* pose) {
  const double h[3] = {w[0] / 2.0, w[1] / 2.0, w[2] / 2.0};
  const double g = sqrt(((1.0 + h[0] * h[0]) + h[1] * h[1]) + h[2] * h[2]);
  const double dq[4] = {1.0 / g, h[0] / g, h[1] / g, h[2] / g};
  const double* q = pose->q;
  double n[4];
  n[0] = dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2] - dq[3] * q[3];
  n[1] = dq[0] * q[1] + dq[1] * q[0] + dq[2] * q[3] - dq[3] * q[2];
  n[2] = dq[0] * q[2] - dq[1] * q[3] + dq[2] * q[0] + dq[3] * q[1];
  n[3] = dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1] + dq[3] * q[0];
  const double len = sqrt(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) + n[3] * n[3]);
  double dR[9], e[3];
  rotation_of(dq, dR);
  for (int k = 0; k < 3; ++k) e[k] = pose->t[k] - c[k];
  for (int k = 0; k < 3; ++k) pose->t[k] = (c[k] + ((dR[3 * k] * e[0] + dR[3 * k + 1] * e[1]) + dR[3 * k + 2] * e[2])) + v[k] / 16.0;
  for (int k = 0; k < 4; ++k) pose->q[k] = n[k] / len;
  rotation_of(pose->q, pose->R);
  return sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) <= eps_rot_rad && sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) / 16.0 <= eps_trans_mm;
}
LMX_PR_FN bool update(const Params& P, const double w[3], const double v[3], const double c[3], Pose* pose) {
  return update_eps(P.eps_rot_rad, P.eps_trans_mm, w, v, c, pose);
}

// ---- control --------------------------------------------------------------------------------------------------------------------------
// What follows pass k (its sums, taken about the centre c under *pose).  True: pass k + 1 runs under the pose this leaves; false: the
// record is final.
LMX_PR_FN bool after_pass(const Params& P, int32_t k, const int64_t a[kSums], const double c[3], Pose* pose, Record* r, Control* ctl) {
  const int32_t n = (int32_t)a[0];
  const double rms = rms_of(a);
  bool more = false;
  if (k == 0) { r->n_pairs_first = n; r->rms_first_mm = rms; }
  if (ctl->final_pass) {
    r->n_pairs_last = n; r->rms_last_mm = rms;
  } else if (n < P.min_pairs) {
    r->status = LOST; r->n_pairs_last = n; r->rms_last_mm = rms;
  } else {
    double w[3], v[3];
    solve(a, w, v);
    const bool converged = update(P, w, v, c, pose);
    r->iterations = k + 1;
    if (converged) r->status = CONVERGED;
    ctl->final_pass = converged || k + 1 >= P.max_iterations;
    more = true;
  }
  if (!more) {
    for (int q = 0; q < 9; ++q) r->R[q] = pose->R[q];
    for (int q = 0; q < 3; ++q) r->t_mm[q] = pose->t[q];
  }
  return more;
}

// ---- the same under a schedule (SCHEDULE above) ---------------------------------------------------------------------------------------------
// The one-stage schedule that is the parameters themselves: what a call without a schedule runs.
LMX_PR_FN Schedule single_stage(const Params& P) {
  Schedule S = {1, 0, {}};
  for (int k = 0; k < kMaxStages; ++k) S.stage[k] = Stage{P.max_dist_mm, P.eps_rot_rad, P.eps_trans_mm, P.max_iterations, P.search_radius, 1, 0};
  return S;
}

// Rows of the debug sums: the most passes a schedule can run.
LMX_PR_FN int32_t schedule_passes(const Schedule& S) {
  int32_t n = 1;
  for (int32_t k = 0; k < S.n_stages; ++k) n += S.stage[k].max_iterations;
  return n;
}

LMX_PR_FN void enter_stage(const Schedule& S, int32_t stage, Record* r, StagedControl* sc) {
  sc->stage = stage;
  sc->k = 0;
  sc->final_pass = stage == S.n_stages - 1 && S.stage[stage].max_iterations == 0;
  r->status = MAX_ITERATIONS;
}

// after_pass under a schedule: what follows pass sc->k of stage sc->stage.  True: another pass runs, of stage sc->stage as this leaves it.
// K (null: no stage is PLANE): the stages' point_shift; pl: the 29 sums of the pass, read when its stage has a shift >= 0.
LMX_PR_FN bool after_pass_plane(const Params& P, const Schedule& S, const PlaneShifts* K, const int64_t a[kSums], const int64_t* pl, const double c[3], Pose* pose, Record* r,
                                StagedControl* sc) {
  const Stage& st = S.stage[sc->stage];
  const bool last = sc->stage == S.n_stages - 1;
  const int32_t n = (int32_t)a[0];
  const double rms = rms_of(a);
  bool more = false;
  if (sc->stage == 0 && sc->k == 0) { r->n_pairs_first = n; r->rms_first_mm = rms; }
  if (sc->final_pass) {
    r->n_pairs_last = n; r->rms_last_mm = rms;
  } else if (n < P.min_pairs) {
    r->status = LOST; r->n_pairs_last = n; r->rms_last_mm = rms;
  } else {
    double w[3], v[3];
    const int32_t shift = K ? K->shift[sc->stage] : -1;
    if (shift >= 0) solve_plane(a, pl, P.min_pairs, shift, w, v);
    else solve(a, w, v);
    const bool converged = update_eps(st.eps_rot_rad, st.eps_trans_mm, w, v, c, pose);
    r->iterations += 1;
    if (converged) r->status = CONVERGED;
    const bool done = converged || sc->k + 1 >= st.max_iterations;
    sc->k += 1;
    if (last) sc->final_pass = done;
    else if (done) enter_stage(S, sc->stage + 1, r, sc);
    more = true;
  }
  if (!more) {
    r->reserved = sc->stage;
    for (int q = 0; q < 9; ++q) r->R[q] = pose->R[q];
    for (int q = 0; q < 3; ++q) r->t_mm[q] = pose->t[q];
  }
  return more;
}

// after_pass_plane without a shift.  Written out, not forwarded: the point-to-point kernels keep the code they had before PLANE existed.
LMX_PR_FN bool after_pass_staged(const Params& P, const Schedule& S, const int64_t a[kSums], const double c[3], Pose* pose, Record* r, StagedControl* sc) {
  const Stage& st = S.stage[sc->stage];
  const bool last = sc->stage == S.n_stages - 1;
  const int32_t n = (int32_t)a[0];
  const double rms = rms_of(a);
  bool more = false;
  if (sc->stage == 0 && sc->k == 0) { r->n_pairs_first = n; r->rms_first_mm = rms; }
  if (sc->final_pass) {
    r->n_pairs_last = n; r->rms_last_mm = rms;
  } else if (n < P.min_pairs) {
    r->status = LOST; r->n_pairs_last = n; r->rms_last_mm = rms;
  } else {
    double w[3], v[3];
    solve(a, w, v);
    const bool converged = update_eps(st.eps_rot_rad, st.eps_trans_mm, w, v, c, pose);
    r->iterations += 1;
    if (converged) r->status = CONVERGED;
    const bool done = converged || sc->k + 1 >= st.max_iterations;
    sc->k += 1;
    if (last) sc->final_pass = done;
    else if (done) enter_stage(S, sc->stage + 1, r, sc);
    more = true;
  }
  if (!more) {
    r->reserved = sc->stage;
    for (int q = 0; q < 9; ++q) r->R[q] = pose->R[q];
    for (int q = 0; q < 3; ++q) r->t_mm[q] = pose->t[q];
  }
  return more;
}

// refine_job under a schedule and the stages' point_shift K (PLANE above).  sums (may be null): [schedule_passes(S)][kSums], one row per pass
// in the order the passes ran; plane_sums (may be null): [schedule_passes(S)][kPlaneSums], the rows of PLANE passes.  normals: the scene's
// normal map, H rows of scene_pitch elements; null when no stage has a shift >= 0.  refine_job_staged is this with every shift -1.
LMX_PR_FN void refine_job_plane(const Params& P, const Schedule& S, const PlaneShifts& K, const uint16_t* crop, int32_t w, int32_t h, int32_t pitch, int32_t rect_x, int32_t rect_y,
                                const uint16_t* scene, const nv::Packed* normals, int32_t W, int32_t H, size_t scene_pitch, int32_t x, int32_t y, Record* r, int64_t* sums,
                                int64_t* plane_sums) {
  int64_t place[kPlaceSums] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int32_t i = 0; i < h; ++i) {
    int32_t Y = 0;
    const bool row_in = dv::scene_row(y, i, H, &Y);
    for (int32_t j = 0; j < w; ++j) {
      const uint16_t t = crop[(size_t)i * (size_t)pitch + j];
      if (t == 0) continue;
      int32_t X = 0;
      const bool met = row_in && dv::scene_col(x, j, W, &X);
      place_pixel(rect_x, rect_y, i, j, t, X, Y, met ? scene[(size_t)Y * scene_pitch + (size_t)X] : (uint16_t)0, place);
    }
  }
  Pose pose;
  Control ctl = {0};
  StagedControl sc = {0, 0, 0};
  double m0[3];
  if (!placement(P, place, m0, &pose, r, &ctl)) return;
  enter_stage(S, 0, r, &sc);
  const Inverse im = inverse_of(P.model), is = inverse_of(P.scene);
  for (int32_t pass = 0;; ++pass) {
    const Stage& st = S.stage[sc.stage];
    const int64_t dmax = dist_ticks(st.max_dist_mm);
    double c[3];
    int64_t C[3], a[kSums], pl[kPlaneSums];
    const bool plane = K.shift[sc.stage] >= 0;
    for (int q = 0; q < kSums; ++q) a[q] = 0;
    for (int q = 0; q < kPlaneSums; ++q) pl[q] = 0;
    centre_of(pose, m0, c, C);
    for (int32_t i = 0; i < h; i += st.stride)
      for (int32_t j = 0; j < w; j += st.stride) {
        const uint16_t t = crop[(size_t)i * (size_t)pitch + j];
        if (t == 0) continue;
        if (plane) pass_pixel_plane_rad(P, st.search_radius, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, scene, normals, W, H, scene_pitch, a, pl);
        else pass_pixel_rad(P, st.search_radius, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, scene, W, H, scene_pitch, a);
      }
    if (sums)
      for (int q = 0; q < kSums; ++q) sums[(size_t)pass * kSums + q] = a[q];
    if (plane_sums && plane)
      for (int q = 0; q < kPlaneSums; ++q) plane_sums[(size_t)pass * kPlaneSums + q] = pl[q];
    if (!after_pass_plane(P, S, &K, a, pl, c, &pose, r, &sc)) return;
  }
}

LMX_PR_FN void refine_job_staged(const Params& P, const Schedule& S, const uint16_t* crop, int32_t w, int32_t h, int32_t pitch, int32_t rect_x, int32_t rect_y,
                                 const uint16_t* scene, int32_t W, int32_t H, size_t scene_pitch, int32_t x, int32_t y, Record* r, int64_t* sums) {
  refine_job_plane(P, S, kNoPlane, crop, w, h, pitch, rect_x, rect_y, scene, nullptr, W, H, scene_pitch, x, y, r, sums, nullptr);
}

// One whole job, pixel by pixel on one thread: the definition the kernel is tested against.  crop: [h][pitch]; scene: H rows of scene_pitch
// elements; sums (may be null): [max_iterations + 1][kSums], pass k's sums at row k, rows of passes that did not run are left alone.
LMX_PR_FN void refine_job(const Params& P, const uint16_t* crop, int32_t w, int32_t h, int32_t pitch, int32_t rect_x, int32_t rect_y, const uint16_t* scene,
                          int32_t W, int32_t H, size_t scene_pitch, int32_t x, int32_t y, Record* r, int64_t* sums) {
  int64_t place[kPlaceSums] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int32_t i = 0; i < h; ++i) {
    int32_t Y = 0;
    const bool row_in = dv::scene_row(y, i, H, &Y);
    for (int32_t j = 0; j < w; ++j) {
      const uint16_t t = crop[(size_t)i * (size_t)pitch + j];
      if (t == 0) continue;
      int32_t X = 0;
      const bool met = row_in && dv::scene_col(x, j, W, &X);
      place_pixel(rect_x, rect_y, i, j, t, X, Y, met ? scene[(size_t)Y * scene_pitch + (size_t)X] : (uint16_t)0, place);
    }
  }
  Pose pose;
  Control ctl = {0};
  double m0[3];
  if (!placement(P, place, m0, &pose, r, &ctl)) return;
  const int64_t dmax = max_dist_ticks(P);
  const Inverse im = inverse_of(P.model), is = inverse_of(P.scene);
  for (int32_t k = 0;; ++k) {
    double c[3];
    int64_t C[3], a[kSums];
    for (int q = 0; q < kSums; ++q) a[q] = 0;
    centre_of(pose, m0, c, C);
    for (int32_t i = 0; i < h; ++i)
      for (int32_t j = 0; j < w; ++j) {
        const uint16_t t = crop[(size_t)i * (size_t)pitch + j];
        if (t != 0) pass_pixel(P, im, is, pose, C, dmax, rect_x, rect_y, i, j, t, scene, W, H, scene_pitch, a);
      }
    if (sums)
      for (int q = 0; q < kSums; ++q) sums[(size_t)k * kSums + q] = a[q];
    if (!after_pass(P, k, a, c, &pose, r, &ctl)) return;
  }
}

// Why a parameter set is refused (null: it is fine): what lmx_pose_refine_matches checks before any device work.
LMX_PR_FN const char* check_params(const Params& P) {
  const Camera* cams[2] = {&P.model, &P.scene};
  for (const Camera* c : cams) {
    if (!(c->fx >= 1.0 / 1024.0 && c->fx <= kMaxPointMm) || !(c->fy >= 1.0 / 1024.0 && c->fy <= kMaxPointMm)) return "focal lengths must lie in [2^-10, 2^20] pixels";
    if (!within(c->cx, kMaxPointMm) || !within(c->cy, kMaxPointMm)) return "principal points must lie in [-2^20, 2^20]";
  }
  if (!(P.max_dist_mm > 0.0 && P.max_dist_mm <= kMaxDistMm)) return "max_dist_mm must lie in (0, 1024]";
  if (!(P.eps_rot_rad >= 0.0) || !(P.eps_trans_mm >= 0.0)) return "eps_rot_rad and eps_trans_mm must be >= 0";
  if (P.max_iterations < 0 || P.max_iterations > kMaxIterations) return "max_iterations must lie in 0 .. 64";
  if (P.min_pairs < 3) return "min_pairs must be >= 3";
  if (P.search_radius < 0 || P.search_radius > kMaxSearchRadius) return "search_radius must lie in 0 .. 2";
  return nullptr;
}

// Why a schedule is refused (null: it is fine), its stages' fields in the ranges check_params gives them.
LMX_PR_FN const char* check_schedule(const Schedule& S) {
  if (S.n_stages < 1 || S.n_stages > kMaxStages) return "a schedule has 1 .. 4 stages";
  for (int32_t k = 0; k < S.n_stages; ++k) {
    const Stage& st = S.stage[k];
    if (!(st.max_dist_mm > 0.0 && st.max_dist_mm <= kMaxDistMm)) return "a stage's max_dist_mm must lie in (0, 1024]";
    if (!(st.eps_rot_rad >= 0.0) || !(st.eps_trans_mm >= 0.0)) return "a stage's eps_rot_rad and eps_trans_mm must be >= 0";
    if (st.max_iterations < 0 || st.max_iterations > kMaxIterations) return "a stage's max_iterations must lie in 0 .. 64";
    if (st.search_radius < 0 || st.search_radius > kMaxSearchRadius) return "a stage's search_radius must lie in 0 .. 2";
    if (st.stride != 1 && st.stride != 2 && st.stride != 4 && st.stride != 8) return "a stage's stride must be 1, 2, 4 or 8";
    if (k + 1 < S.n_stages && st.max_iterations < 1) return "a stage that is not the last needs max_iterations >= 1";
  }
  return nullptr;
}

// Why a point_shift list is refused (null: it is fine): what lmx_depth_templates_set_refine_plane checks.
LMX_PR_FN const char* check_plane(const int32_t* point_shift, int32_t n_stages) {
  if (n_stages < 0 || n_stages > kMaxStages) return "n_stages must lie in 0 .. 4";
  if (n_stages > 0 && !point_shift) return "point_shift is null with n_stages > 0";
  for (int32_t k = 0; k < n_stages; ++k)
    if (point_shift[k] < -1 || point_shift[k] > kMaxPointShift) return "a point_shift must lie in -1 .. 20";
  return nullptr;
}

}  // namespace pr
}  // namespace lmx
