// Verification of a refined pose against the scene's voxel occupancy (lmx_pose_verify_matches, include/lmx.h): the arithmetic of one model
// point, one scene pixel and one job, shared by the HIP kernel (lmx_verify.hip, k_pose_verify) and -- compiled with LMX_PR_HOST -- by plain
// CPU builds (tests/cpp/pose_verify_host.cpp).  The stage stands where the reference runs hypothesisVerification (src/rgbdDetector.cpp:
// 1457-1506: a PCL octree of 4 mm voxels over the cluster's scene cloud, the share of the posed model cloud's points that fall in an
// occupied voxel, the cluster erased below a threshold).  PCL is not part of the reference, and its octree anchors the voxels at a bounding
// box that depends on the order of insertion, so the definition below is this repository's own: a voxel lattice anchored at the camera
// origin.  Points, poses and ticks are those of lmx_pose_refine.hpp (pr::back, pr::mat_point, pr::ticks_of, pr::within); build with
// -ffp-contract=off.  This comment is the specification; tests/pose_verify_cases.py restates it in numpy.
//
// INPUT  a template crop t[h][w] with its rect corner (rect_x, rect_y), the model camera and the scene camera, the scene s[H][W], a pose
//   (R, t_mm) -- the R and t_mm of the match's lmx_pose_refine_t --, voxel_mm in [0.25, 64], roi_margin in 0..64 pixels.
//   vt = llrint(16 voxel_mm): the voxel's side in ticks (1/16 mm), 4..1024.
//   floor_div(a, b), b > 0: the quotient rounded towards minus infinity.  key(P) = (floor_div(P.x, vt), floor_div(P.y, vt), floor_div(P.z, vt)).
//
// MODEL POINTS  for every crop pixel (i, j) with t = crop[i][j] != 0:  M = back(model, rect_x + j, rect_y + i, t),  p = R M + t_mm with the
//   row expression of pr::mat_point.  The point is TESTED iff p.z >= 1 and |p.x|, |p.y|, |p.z| <= 2^20 and, with
//   xr = rint((p.x fx_s) / p.z + cx_s), yr = rint((p.y fy_s) / p.z + cy_s), also |xr|, |yr| <= 2^20.  A tested point has the key
//   K = key(ticks_of(p)) and the projection (xr, yr) as integers.   n_model = #{t != 0}, n_tested = #tested.
//
// GRID  lo, hi: the component-wise minimum and maximum of K over the tested points; dims = hi - lo + 1; cells = dims.x dims.y dims.z as an
//   exact integer (the record holds min(cells, 2^31 - 1)).  n_tested == 0: status EMPTY, every other count 0, roi 0.
//   cells > kMaxCells = 2^18 (a bitmap of 32 KiB, the kernel's LDS array): status GRID_TOO_LARGE, n_occupied = n_scene = 0, rate = 0.
//   The cell of a key k inside [lo, hi]:  ((k.z - lo.z) dims.y + (k.y - lo.y)) dims.x + (k.x - lo.x).
//
// REGION OF INTEREST  x0 = max(min xr - roi_margin, 0), x1 = min(max xr + roi_margin, W - 1), y0, y1 likewise with H, the minima and maxima
//   over the tested points.  The record's roi is (x0, y0, x1 - x0 + 1, y1 - y0 + 1), or (0, 0, 0, 0) when x1 < x0 or y1 < y0: the empty ROI.
//
// SCENE POINTS  for every pixel (X, Y) of the ROI with s = scene[Y][X] != 0:  Q = back(scene, X, Y, s); the pixel is skipped unless
//   |Q.x|, |Q.y| <= 2^21; its key is key(ticks_of(Q)); if the key lies inside [lo, hi] its cell is marked.  n_scene = the number of pixels
//   that mark a cell (not the number of distinct cells).
//
// RESULT  n_occupied = the tested model points whose cell is marked.  rate = n_model > 0 ? (double)n_occupied / (double)n_model : 0 -- the
//   divisor is n_model, as in the reference.  status OK.  Everything is an integer apart from p, Q, the two projections and the final
//   quotient; marking is idempotent and the counts are sums, so the result does not depend on any order of evaluation.
//   Bounds: |ticks| <= 2^25 and |key| <= 2^23 fit an int32; a cell index is below 2^18; the counts are at most 2^28 pixels.
#pragma once

#include "lmx_pose_refine.hpp"

namespace lmx {
namespace pv {

constexpr int32_t kMaxCells = 1 << 18;
constexpr int32_t kBitmapWords = kMaxCells / 32;   // 32 KiB
constexpr double kMinVoxelMm = 0.25, kMaxVoxelMm = 64.0;
constexpr int32_t kMaxRoiMargin = 64;
constexpr double kMaxRotationEntry = 2.0;

enum Status : int32_t { NONE = 0, OK = 1, EMPTY = 2, GRID_TOO_LARGE = 3 };

struct Params {
  pr::Camera model, scene;
  double voxel_mm;
  int32_t roi_margin, pad;
};
struct Record {   // the bytes of lmx_pose_verify_t
  double rate;
  int32_t n_model, n_tested, n_occupied, n_scene, cells, status;
  int32_t roi[4];
};
// What the first walk over the crop leaves: the extent of the keys and of the projections, the two counts.
struct Bounds {
  int32_t lo[3], hi[3];
  int32_t xmin, xmax, ymin, ymax;
  int32_t n_model, n_tested;
};
// What the later phases need of it.
struct Grid {
  int32_t lo[3], dims[3];
  int32_t x0, y0, roi_w, roi_h;   // roi_w == 0 or roi_h == 0: empty
};

LMX_PR_FN int32_t voxel_ticks(const Params& P) { return (int32_t)llrint(16.0 * P.voxel_mm); }

LMX_PR_FN int32_t floor_div(int32_t a, int32_t b) {
  const int32_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

LMX_PR_FN void key_of(const double p[3], int32_t vt, int32_t K[3]) {
  for (int k = 0; k < 3; ++k) K[k] = floor_div((int32_t)pr::ticks_of(p[k]), vt);
}

LMX_PR_FN void bounds_init(Bounds* b) {
  for (int k = 0; k < 3; ++k) { b->lo[k] = INT32_MAX; b->hi[k] = INT32_MIN; }
  b->xmin = b->ymin = INT32_MAX;
  b->xmax = b->ymax = INT32_MIN;
  b->n_model = b->n_tested = 0;
}

LMX_PR_FN void bounds_merge(Bounds* b, const Bounds& o) {
  for (int k = 0; k < 3; ++k) {
    b->lo[k] = o.lo[k] < b->lo[k] ? o.lo[k] : b->lo[k];
    b->hi[k] = o.hi[k] > b->hi[k] ? o.hi[k] : b->hi[k];
  }
  b->xmin = o.xmin < b->xmin ? o.xmin : b->xmin;
  b->ymin = o.ymin < b->ymin ? o.ymin : b->ymin;
  b->xmax = o.xmax > b->xmax ? o.xmax : b->xmax;
  b->ymax = o.ymax > b->ymax ? o.ymax : b->ymax;
  b->n_model += o.n_model;
  b->n_tested += o.n_tested;
}

// The model point of crop pixel (i, j), t != 0, under the pose: true when it is tested, with its key and its projection.
LMX_PR_FN bool model_point(const Params& P, const pr::Inverse& im, const double R[9], const double t_mm[3], int32_t vt, int32_t rect_x, int32_t rect_y, int32_t i,
                           int32_t j, uint16_t t, int32_t K[3], int32_t* X, int32_t* Y) {
  double M[3], p[3];
  pr::back(P.model, im, (int64_t)rect_x + j, (int64_t)rect_y + i, t, M);
  pr::mat_point(R, M, t_mm, p);
  if (!(p[2] >= 1.0) || !pr::within(p[0], pr::kMaxPointMm) || !pr::within(p[1], pr::kMaxPointMm) || !pr::within(p[2], pr::kMaxPointMm)) return false;
  const double xr = rint((p[0] * P.scene.fx) / p[2] + P.scene.cx), yr = rint((p[1] * P.scene.fy) / p[2] + P.scene.cy);
  if (!pr::within(xr, pr::kMaxPointMm) || !pr::within(yr, pr::kMaxPointMm)) return false;
  key_of(p, vt, K);
  *X = (int32_t)xr;
  *Y = (int32_t)yr;
  return true;
}

// Phase 1, one crop pixel t != 0.
LMX_PR_FN void bounds_pixel(const Params& P, const pr::Inverse& im, const double R[9], const double t_mm[3], int32_t vt, int32_t rect_x, int32_t rect_y, int32_t i,
                            int32_t j, uint16_t t, Bounds* b) {
  int32_t K[3], X, Y;
  b->n_model += 1;
  if (!model_point(P, im, R, t_mm, vt, rect_x, rect_y, i, j, t, K, &X, &Y)) return;
  b->n_tested += 1;
  for (int k = 0; k < 3; ++k) {
    b->lo[k] = K[k] < b->lo[k] ? K[k] : b->lo[k];
    b->hi[k] = K[k] > b->hi[k] ? K[k] : b->hi[k];
  }
  b->xmin = X < b->xmin ? X : b->xmin;
  b->xmax = X > b->xmax ? X : b->xmax;
  b->ymin = Y < b->ymin ? Y : b->ymin;
  b->ymax = Y > b->ymax ? Y : b->ymax;
}

// The record's start and the grid from the bounds of the whole crop.  False: EMPTY or GRID_TOO_LARGE, the record is final.
LMX_PR_FN bool grid_of(const Params& P, const Bounds& b, int32_t W, int32_t H, Grid* g, Record* r) {
  r->rate = 0.0;
  r->n_model = b.n_model;
  r->n_tested = b.n_tested;
  r->n_occupied = r->n_scene = r->cells = 0;
  r->roi[0] = r->roi[1] = r->roi[2] = r->roi[3] = 0;
  r->status = EMPTY;
  if (b.n_tested == 0) return false;
  int64_t cells = 1;   // dims < 2^25: the product of two fits; it is cut off at 2^31 - 1 before the third
  for (int k = 0; k < 3; ++k) {
    g->lo[k] = b.lo[k];
    g->dims[k] = b.hi[k] - b.lo[k] + 1;
    cells = cells * (int64_t)g->dims[k];
    if (cells > (int64_t)INT32_MAX) cells = INT32_MAX;
  }
  r->cells = (int32_t)cells;
  const int64_t x0 = (int64_t)b.xmin - P.roi_margin, x1 = (int64_t)b.xmax + P.roi_margin, y0 = (int64_t)b.ymin - P.roi_margin, y1 = (int64_t)b.ymax + P.roi_margin;
  const int64_t cx0 = x0 < 0 ? 0 : x0, cx1 = x1 > (int64_t)W - 1 ? (int64_t)W - 1 : x1, cy0 = y0 < 0 ? 0 : y0, cy1 = y1 > (int64_t)H - 1 ? (int64_t)H - 1 : y1;
  const bool some = cx1 >= cx0 && cy1 >= cy0;
  g->x0 = some ? (int32_t)cx0 : 0;
  g->y0 = some ? (int32_t)cy0 : 0;
  g->roi_w = some ? (int32_t)(cx1 - cx0 + 1) : 0;
  g->roi_h = some ? (int32_t)(cy1 - cy0 + 1) : 0;
  r->roi[0] = g->x0; r->roi[1] = g->y0; r->roi[2] = g->roi_w; r->roi[3] = g->roi_h;
  r->status = GRID_TOO_LARGE;
  if (cells > (int64_t)kMaxCells) return false;
  r->status = OK;
  return true;
}

LMX_PR_FN int32_t bitmap_words(const Grid& g) { return (g.dims[0] * g.dims[1] * g.dims[2] + 31) / 32; }

// The cell of a key, or -1 when the key lies outside [lo, hi].
LMX_PR_FN int32_t cell_of(const Grid& g, const int32_t K[3]) {
  const int64_t a = (int64_t)K[0] - g.lo[0], b = (int64_t)K[1] - g.lo[1], c = (int64_t)K[2] - g.lo[2];
  if (a < 0 || a >= g.dims[0] || b < 0 || b >= g.dims[1] || c < 0 || c >= g.dims[2]) return -1;
  return ((int32_t)c * g.dims[1] + (int32_t)b) * g.dims[0] + (int32_t)a;
}

// Phase 3, one ROI pixel s != 0 at (X, Y): the cell it marks, or -1.
LMX_PR_FN int32_t scene_cell(const Params& P, const pr::Inverse& is, const Grid& g, int32_t vt, int32_t X, int32_t Y, uint16_t s) {
  double Q[3];
  pr::back(P.scene, is, (int64_t)X, (int64_t)Y, s, Q);
  if (!pr::within(Q[0], pr::kMaxScenePointMm) || !pr::within(Q[1], pr::kMaxScenePointMm)) return -1;
  int32_t K[3];
  key_of(Q, vt, K);
  return cell_of(g, K);
}

// Phase 4, one crop pixel t != 0: the cell of its point, recomputed from phase 1's expressions, or -1 when the point is not tested.
LMX_PR_FN int32_t model_cell(const Params& P, const pr::Inverse& im, const double R[9], const double t_mm[3], const Grid& g, int32_t vt, int32_t rect_x, int32_t rect_y,
                             int32_t i, int32_t j, uint16_t t) {
  int32_t K[3], X, Y;
  if (!model_point(P, im, R, t_mm, vt, rect_x, rect_y, i, j, t, K, &X, &Y)) return -1;
  return cell_of(g, K);
}

LMX_PR_FN void finish(int32_t n_scene, int32_t n_occupied, Record* r) {
  r->n_scene = n_scene;
  r->n_occupied = n_occupied;
  r->rate = r->n_model > 0 ? (double)n_occupied / (double)r->n_model : 0.0;
}

// One whole job, pixel by pixel on one thread: the definition the kernel is tested against.  crop: [h][pitch]; scene: H rows of scene_pitch
// elements; bitmap: kBitmapWords words of scratch.
LMX_PR_FN void verify_job(const Params& P, const uint16_t* crop, int32_t w, int32_t h, int32_t pitch, int32_t rect_x, int32_t rect_y, const uint16_t* scene, int32_t W,
                          int32_t H, size_t scene_pitch, const double R[9], const double t_mm[3], uint32_t* bitmap, Record* r) {
  const int32_t vt = voxel_ticks(P);
  const pr::Inverse im = pr::inverse_of(P.model), is = pr::inverse_of(P.scene);
  Bounds b;
  bounds_init(&b);
  for (int32_t i = 0; i < h; ++i)
    for (int32_t j = 0; j < w; ++j) {
      const uint16_t t = crop[(size_t)i * (size_t)pitch + j];
      if (t != 0) bounds_pixel(P, im, R, t_mm, vt, rect_x, rect_y, i, j, t, &b);
    }
  Grid g;
  if (!grid_of(P, b, W, H, &g, r)) return;
  const int32_t words = bitmap_words(g);
  for (int32_t k = 0; k < words; ++k) bitmap[k] = 0;
  int32_t n_scene = 0, n_occupied = 0;
  for (int32_t Y = g.y0; Y < g.y0 + g.roi_h; ++Y)
    for (int32_t X = g.x0; X < g.x0 + g.roi_w; ++X) {
      const uint16_t s = scene[(size_t)Y * scene_pitch + (size_t)X];
      if (s == 0) continue;
      const int32_t cell = scene_cell(P, is, g, vt, X, Y, s);
      if (cell < 0) continue;
      bitmap[cell >> 5] |= 1u << (cell & 31);
      n_scene += 1;
    }
  for (int32_t i = 0; i < h; ++i)
    for (int32_t j = 0; j < w; ++j) {
      const uint16_t t = crop[(size_t)i * (size_t)pitch + j];
      if (t == 0) continue;
      const int32_t cell = model_cell(P, im, R, t_mm, g, vt, rect_x, rect_y, i, j, t);
      if (cell >= 0) n_occupied += (int32_t)((bitmap[cell >> 5] >> (cell & 31)) & 1u);
    }
  finish(n_scene, n_occupied, r);
}

// Why a parameter set is refused (null: it is fine): what lmx_pose_verify_matches checks before any device work.
LMX_PR_FN const char* check_params(const Params& P) {
  const pr::Camera* cams[2] = {&P.model, &P.scene};
  for (const pr::Camera* c : cams) {
    if (!(c->fx >= 1.0 / 1024.0 && c->fx <= pr::kMaxPointMm) || !(c->fy >= 1.0 / 1024.0 && c->fy <= pr::kMaxPointMm)) return "focal lengths must lie in [2^-10, 2^20] pixels";
    if (!pr::within(c->cx, pr::kMaxPointMm) || !pr::within(c->cy, pr::kMaxPointMm)) return "principal points must lie in [-2^20, 2^20]";
  }
  if (!(P.voxel_mm >= kMinVoxelMm && P.voxel_mm <= kMaxVoxelMm)) return "voxel_mm must lie in [0.25, 64]";
  if (P.roi_margin < 0 || P.roi_margin > kMaxRoiMargin) return "roi_margin must lie in 0 .. 64";
  return nullptr;
}

// Why a pose is refused (null: it is fine): an entry that is not finite, |R[k]| > 2 or |t_mm[k]| > 2^20.
LMX_PR_FN const char* check_pose(const double R[9], const double t_mm[3]) {
  for (int k = 0; k < 9; ++k)
    if (!pr::within(R[k], kMaxRotationEntry)) return "an entry of R is not finite or beyond +-2";
  for (int k = 0; k < 3; ++k)
    if (!pr::within(t_mm[k], pr::kMaxPointMm)) return "an entry of t_mm is not finite or beyond +-2^20";
  return nullptr;
}

// The reference's erase rule, the other way round: kept unless rate < thresh (a NaN threshold keeps).
LMX_PR_FN bool keep(const Record& r, double thresh) { return r.status == OK && !(r.rate < thresh); }

}  // namespace pv
}  // namespace lmx
