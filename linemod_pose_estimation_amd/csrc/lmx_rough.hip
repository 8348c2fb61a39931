// Rough pose per cluster on the device (lmx_rough_pose_chain_on, include/lmx.h): the reference's getRoughPoseByClustering in front of the
// refine and verify bodies of lmx_verify.hip.  The arithmetic is lmx_rough_pose.hpp (groups, winner, means) and lmx_mesh_raster.hpp (the
// render); this file is the model object and the parallel shape.  Four kernels per call, every dependency a kernel boundary on one stream,
// no workgroup waits for another, every store an ordinary vector store:
//
//   k_rough_group   one 64-lane workgroup (one wave) per cluster slot, a grid of cap_clusters; a slot at or above n_live leaves without a
//                   store.  The frames and the member checks spread over the lanes (ORs: no order), then first fit member by member: 64
//                   members' rotations staged in LDS, the lanes test one member against 64 fronts at a time (fronts in LDS, one array per
//                   matrix entry), a ballot whose lowest lane in the earliest chunk wins.  Lane 0 runs the emulated std::sort over the
//                   group sizes in LDS.  The sums: 64 members' table rows per pass, one lane each, added in member order by every lane
//                   alike from shuffles.  Lane 0 stores the record, the slot's view (the 10 doubles the setup reads) and its job; lanes
//                   0..31 clear the slot's rasteriser state.  66 vector registers, 78 scalar, 46.5 KiB LDS (the fronts: 36 KiB), 1024 bytes of scratch
//                   per lane: the emulated sort's explicit stack, which lane 0 alone touches.
//   k_rough_setup   k_mesh_setup's body (lmx_mesh_device.hpp: mesh_setup, the one both kernels call) per (slot, triangle) for the slots
//                   that have a view.  44 vector registers, 62 scalar, no scratch.
//   k_rough_raster  k_mesh_raster's walk (mesh_tile_walk, without the gray) per (slot, 32x8 tile of the slot's WINDOW): the window is the union box the setup folded, stored at
//                   the slot's place in the arena with rows of crop_pitch(width) -- a 640x480 frame per slot would be 2.5 GB for 4096 slots.
//                   Tiles beyond the window leave at once.  Silhouette box and pixel count: LDS atomics, one global atomic set per
//                   workgroup.  53 vector registers, 54 scalar, no scratch, 24.0 KiB LDS.
//   k_rough_finish  one lane per slot: the status the render gives (INVALID_VIEW, EMPTY, WINDOW_TOO_LARGE), rect and n_model, the slot's
//                   crop table entry (the whole window: zero pixels count nowhere in the refine and verify definitions) and its job.  24 vector
//                   registers, 34 scalar, no scratch.
#include <cmath>
#include <cstring>
#include <vector>

#include "lmx_rough.hpp"
#include "lmx_depth_verify.hpp"
#include "lmx_mesh_device.hpp"

namespace lmx {
namespace {

struct GroupArgs {
  rp::StageArgs a;
  const rp::View* views;
  int32_t n_views;
  double* slot_view;
  int32_t* state;
  rp::Job* jobs;
};

__global__ __launch_bounds__(64) void k_rough_group(const GroupArgs g) {
  __shared__ double s_front[9][rp::kMaxGroups];
  __shared__ double s_mR[9][64];
  __shared__ int32_t s_size[rp::kMaxGroups], s_frontm[rp::kMaxGroups], s_idx[rp::kMaxGroups];
  __shared__ int32_t s_win;
  const pc::Lists& L = g.a.L;
  const int lane = threadIdx.x;
  const uint32_t k = blockIdx.x, n_live = pc::n_live(L);
  if (k == 0 && lane == 0) {
    g.a.chain_header[pc::C_LIVE] = n_live;
    const uint32_t hf = pc::header_flags(L);
    if (hf) atomicOr(&g.a.chain_header[pc::C_FLAGS], hf);
  }
  if (k >= n_live) return;
  int32_t claims = 0, first = INT32_MAX;
  for (int32_t f = lane; f < L.n_frames; f += 64)
    if (pc::frame_claims(L, f, k)) { claims += 1; first = f < first ? f : first; }
  claims = __shfl(wave_sum(claims), 0, 64);
  first = __shfl(wave_min(first), 0, 64);
  // the branches depend on k and on device memory alone: the wave stays together
  rp::Slot s = rp::slot_from_claims(L, g.a.class_index, k, claims, first, [&](const pc::Frame& fr, const pc::Cluster& c, int32_t first_class) {
    const rp::Scan one = rp::scan_of_lane(L, fr, c, g.n_views, first_class, lane, 64);
    return rp::Scan{__any(one.bad_member) ? 1 : 0, __any(one.bad_view) ? 1 : 0, __any(one.mixed) ? 1 : 0};
  });
  rp::Record rec;
  rp::record_zero(&rec);
  if (s.state == pc::JOB) {
    const int32_t mc = s.member_count;
    const size_t mb = (size_t)s.member_begin;
    int32_t n_groups = 0, first_bad = -1;
    for (int32_t base = 0; base < mc && first_bad < 0; base += 64) {
      const int32_t n = mc - base < 64 ? mc - base : 64;
      __syncthreads();   // the previous pass's rows have been read
      int32_t my_match = -1;
      if (lane < n) {
        my_match = s.match_begin + L.members[mb + (size_t)(base + lane)];
        const double* R = g.views[L.matches[my_match].template_id].R;
        for (int j = 0; j < 9; ++j) s_mR[j][lane] = R[j];
      }
      __syncthreads();
      for (int32_t i = 0; i < n; ++i) {
        double Rp[9];
        for (int j = 0; j < 9; ++j) Rp[j] = s_mR[j][i];
        const int32_t match_i = __shfl(my_match, i, 64);
        int32_t found = -1;
        for (int32_t c0 = 0; c0 < n_groups; c0 += 64) {
          const int32_t gi = c0 + lane;
          bool hit = false;
          if (gi < n_groups) {
            double F[9];
            for (int j = 0; j < 9; ++j) F[j] = s_front[j][gi];
            hit = rp::trace_dot(Rp, F) > g.a.trace_min;
          }
          const unsigned long long bal = __ballot(hit);
          if (bal) { found = c0 + __ffsll(bal) - 1; break; }
        }
        if (found < 0) {
          if (n_groups == rp::kMaxGroups) { first_bad = base + i; break; }
          found = n_groups;
          if (lane < 9) s_front[lane][found] = s_mR[lane][i];
          if (lane == 0) { s_size[found] = 0; s_frontm[found] = match_i; }
          n_groups += 1;
          __syncthreads();   // one wave: orders the LDS stores in front of the next member's loads
        }
        if (lane == 0) { s_size[found] += 1; g.a.member_group[mb + (size_t)(base + i)] = found; }
      }
    }
    if (first_bad >= 0) {
      for (int32_t q = first_bad + lane; q < mc; q += 64) g.a.member_group[mb + (size_t)q] = -1;
      rp::record_too_many(mc, &rec);
    } else {
      __syncthreads();   // s_size; and member_group, which the lanes of this workgroup read back
      if (lane == 0) s_win = rp::winning_group(s_size, n_groups, s_idx);
      __syncthreads();
      const int32_t win = s_win;
      rp::Sums sums;
      rp::sums_init(&sums);
      for (int32_t base = 0; base < mc; base += 64) {
        const int32_t p = base + lane;
        bool in = false;
        double q0 = 0, q1 = 0, q2 = 0, q3 = 0, dist = 0, D = 0, ori = 0;
        int32_t mx = 0, my = 0;
        if (p < mc && g.a.member_group[mb + (size_t)p] == win) {
          in = true;
          const pc::Match m = L.matches[s.match_begin + L.members[mb + (size_t)p]];
          const rp::View* v = g.views + m.template_id;
          q0 = v->q[0]; q1 = v->q[1]; q2 = v->q[2]; q3 = v->q[3]; dist = v->distance; D = v->D; ori = v->ori_dist;
          mx = m.x; my = m.y;
        }
        unsigned long long mask = __ballot(in);
        while (mask) {   // in member order; every lane adds the same
          const int i = __ffsll(mask) - 1;
          mask &= mask - 1;
          const double q[4] = {__shfl(q0, i, 64), __shfl(q1, i, 64), __shfl(q2, i, 64), __shfl(q3, i, 64)};
          rp::sums_add(&sums, q, __shfl(dist, i, 64), __shfl(D, i, 64), __shfl(ori, i, 64), __shfl(mx, i, 64), __shfl(my, i, 64));
        }
      }
      if (!rp::record_of_sums(sums, mc, n_groups, win, s_frontm[win], &rec)) {
        rp::record_zero(&rec);
        s.state = pc::NO_JOB_BOUNDS; s.flags |= pc::FLAG_BOUNDS;
      }
    }
  }
  if (lane < kMeshStateWords) g.state[(size_t)k * kMeshStateWords + lane] = mesh_state_clear(lane, 8);   // the union box and level 0's
  const bool run = s.state == pc::JOB && rec.status == rp::OK;
  if (run && lane < 10) g.slot_view[(size_t)k * 10 + lane] = lane < 9 ? rec.R[lane] : rec.distance;
  if (lane == 0) {
    g.a.rough[k] = rec;
    g.jobs[k] = rp::Job{run ? 1 : 0, s.frame, rec.x, rec.y, 0, 0, 0, 0};
    const uint32_t flags = s.flags | ((s.state == pc::JOB && !run) ? rp::FLAG_ROUGH : 0u);
    if (flags) atomicOr(&g.a.chain_header[pc::C_FLAGS], flags);
  }
}

struct RenderArgs {
  const uint32_t* header;
  uint64_t cap_clusters;
  const rp::Job* jobs;
  const double* tri;
  int32_t n_tri;
  mr::Camera cam;
  const double* slot_view;
  mr::Tri* work;
  int32_t* state;
  uint16_t* window;
  size_t win_stride;
  int32_t win_w, win_h;
};

__global__ __launch_bounds__(256) void k_rough_setup(const RenderArgs a) {
  const uint32_t v = blockIdx.x;   // the slot in x: up to 2^16 of them
  if (v >= pc::n_live(a.header, a.cap_clusters) || !a.jobs[v].run) return;
  const int t = blockIdx.y * 256 + threadIdx.x;
  mesh_setup(a.tri, a.n_tri, a.cam, a.slot_view + (size_t)v * 10, a.work + (size_t)v * a.n_tri, a.state + (size_t)v * kMeshStateWords, t);
}

// The slot's window, or false: no view, an invalid view, no triangle on the image, a union box larger than the model's window.
__device__ __forceinline__ bool slot_window(const RenderArgs& a, uint32_t v, int* ux0, int* uy0, int* uw, int* uh) {
  const int32_t* st = a.state + (size_t)v * kMeshStateWords;
  if (st[MS_INVALID] || st[MS_UNION + 2] < 0) return false;
  *ux0 = st[MS_UNION + 0]; *uy0 = st[MS_UNION + 1];
  *uw = st[MS_UNION + 2] - *ux0 + 1; *uh = st[MS_UNION + 3] - *uy0 + 1;   // inside the camera's image: setup_triangle clamps the boxes
  return *uw <= a.win_w && *uh <= a.win_h;
}

__global__ __launch_bounds__(256) void k_rough_raster(const RenderArgs a) {
  __shared__ mr::Tri s_tri[256];
  __shared__ int s_wave[4];
  __shared__ int s_sbox[4], s_count;
  const uint32_t v = blockIdx.x;   // the slot in x: up to 2^16 of them
  const int tid = threadIdx.x;
  if (v >= pc::n_live(a.header, a.cap_clusters) || !a.jobs[v].run) return;
  int ux0, uy0, uw, uh;
  if (!slot_window(a, v, &ux0, &uy0, &uw, &uh)) return;
  const int wx0 = blockIdx.y * MR_TW, wy0 = blockIdx.z * MR_TH;
  if (wx0 >= uw || wy0 >= uh) return;
  const int pitch = dv::crop_pitch(uw);
  const int wx = wx0 + (tid & (MR_TW - 1)), wy = wy0 + tid / MR_TW;
  const int x = ux0 + wx, y = uy0 + wy;
  const bool inside = wx < uw && wy < uh;
  const int tx0 = ux0 + wx0, ty0 = uy0 + wy0;
  const int tx1 = min(tx0 + MR_TW, ux0 + uw) - 1, ty1 = min(ty0 + MR_TH, uy0 + uh) - 1;
  if (tid < 4) s_sbox[tid] = (tid & 2) ? -1 : MR_BIG;
  if (tid == 4) s_count = 0;
  const double best_z = mesh_tile_walk<false>(a.work + (size_t)v * a.n_tri, a.n_tri, tx0, ty0, tx1, ty1, x, y, inside, s_tri, s_wave).z;
  const bool cov = inside && best_z < INFINITY;
  if (wx < pitch && wy < uh) a.window[(size_t)v * a.win_stride + (size_t)wy * pitch + wx] = cov ? mr::depth_mm(best_z) : (uint16_t)0;   // past uw: the padding
  if (cov) {
    atomicMin(&s_sbox[0], x); atomicMin(&s_sbox[1], y); atomicMax(&s_sbox[2], x); atomicMax(&s_sbox[3], y);
    atomicAdd(&s_count, 1);
  }
  __syncthreads();
  int32_t* st = a.state + (size_t)v * kMeshStateWords;
  if (tid < 4 && s_sbox[2] >= 0) {
    if (tid < 2) atomicMin(&st[MS_LEVEL + tid], s_sbox[tid]);
    else atomicMax(&st[MS_LEVEL + tid], s_sbox[tid]);
  }
  if (tid == 4 && s_count) atomicAdd(&st[MS_COUNT], s_count);
}

struct FinishArgs {
  RenderArgs r;
  rp::Record* rough;
  rp::CropEntry* crops;
  rp::Job* jobs;
  uint32_t* chain_header;
};

__global__ __launch_bounds__(64) void k_rough_finish(const FinishArgs f) {
  const RenderArgs& a = f.r;
  const uint32_t v = blockIdx.x * 64 + threadIdx.x;
  if (v >= pc::n_live(a.header, a.cap_clusters)) return;
  rp::CropEntry entry = {nullptr, 0, 0, 0, 0};
  rp::Job job = f.jobs[v];
  if (job.run) {
    const int32_t* st = a.state + (size_t)v * kMeshStateWords;
    int ux0 = 0, uy0 = 0, uw = 0, uh = 0;
    int32_t status = rp::OK;
    if (st[MS_INVALID]) status = rp::INVALID_VIEW;
    else if (st[MS_UNION + 2] < 0) status = rp::EMPTY;
    else if (!slot_window(a, v, &ux0, &uy0, &uw, &uh)) status = rp::WINDOW_TOO_LARGE;
    else if (st[MS_LEVEL + 2] < 0) status = rp::EMPTY;
    rp::Record* r = f.rough + v;
    r->status = status;
    if (status == rp::OK) {
      const int32_t sx0 = st[MS_LEVEL + 0], sy0 = st[MS_LEVEL + 1];
      r->rect[0] = sx0; r->rect[1] = sy0; r->rect[2] = st[MS_LEVEL + 2] - sx0 + 1; r->rect[3] = st[MS_LEVEL + 3] - sy0 + 1;
      r->n_model = st[MS_COUNT];
      entry = rp::CropEntry{a.window + (size_t)v * a.win_stride, uw, uh, dv::crop_pitch(uw), 0};
      job.x += ux0 - sx0; job.y += uy0 - sy0; job.rect_x = ux0; job.rect_y = uy0; job.lat_x = sx0 - ux0; job.lat_y = sy0 - uy0;
      atomicAdd(&f.chain_header[rp::C_ROUGH_OK], 1u);
    } else {
      job.run = 0;
      atomicOr(&f.chain_header[pc::C_FLAGS], rp::FLAG_ROUGH);
    }
    f.jobs[v] = job;
  }
  f.crops[v] = entry;
}

}  // namespace

void launch_rough_stage(hipStream_t s, const lmx_rough_model* m, const rp::StageArgs& a) {
  const unsigned n_slots = (unsigned)a.L.cap_clusters;
  const GroupArgs g = {a, m->d_views, m->n_views, m->d_slot_view, m->d_state, m->d_jobs};
  hipLaunchKernelGGL(k_rough_group, dim3(n_slots), dim3(64), 0, s, g);
  const RenderArgs r = {a.L.header, a.L.cap_clusters, m->d_jobs, m->d_tri, m->n_tri, m->cam, m->d_slot_view, m->d_work, m->d_state, m->d_window, m->win_stride,
                        m->win_w, m->win_h};
  hipLaunchKernelGGL(k_rough_setup, dim3(n_slots, (unsigned)((m->n_tri + 255) / 256)), dim3(256), 0, s, r);   // <= 2^14 blocks of triangles
  const dim3 grid(n_slots, (unsigned)((m->win_w + MR_TW - 1) / MR_TW), (unsigned)((m->win_h + MR_TH - 1) / MR_TH));   // <= 512 x 2048 tiles
  hipLaunchKernelGGL(k_rough_raster, grid, dim3(256), 0, s, r);
  const FinishArgs f = {r, a.rough, m->d_crops, m->d_jobs, a.chain_header};
  hipLaunchKernelGGL(k_rough_finish, dim3((n_slots + 63) / 64), dim3(64), 0, s, f);
}

}  // namespace lmx

namespace {
void rough_model_release(lmx_rough_model* m) {
  (void)hipFree(m->d_tri); (void)hipFree(m->d_views); (void)hipFree(m->d_slot_view); (void)hipFree(m->d_state); (void)hipFree(m->d_work);
  (void)hipFree(m->d_window); (void)hipFree(m->d_crops); (void)hipFree(m->d_jobs);
  if (m->done) (void)hipEventDestroy(m->done);
  delete m;
}

lmx_status rough_model_fill(lmx_rough_model* m, const double* triangles, const std::vector<lmx::rp::View>& table) {
  using namespace lmx;
  HIP_RETURN(hipSetDevice(m->device));
  const size_t S = (size_t)m->cap_slots;
  const size_t b_tri = (size_t)m->n_tri * 9 * sizeof(double), b_views = table.size() * sizeof(rp::View), b_sv = S * 10 * sizeof(double),
               b_state = S * kMeshStateWords * sizeof(int32_t), b_work = S * (size_t)m->n_tri * sizeof(mr::Tri), b_win = S * m->win_stride * sizeof(uint16_t),
               b_crops = S * sizeof(rp::CropEntry), b_jobs = S * sizeof(rp::Job);
  HIP_RETURN(hipMalloc(&m->d_tri, b_tri));
  HIP_RETURN(hipMalloc(&m->d_views, b_views));
  HIP_RETURN(hipMalloc(&m->d_slot_view, b_sv));
  HIP_RETURN(hipMalloc(&m->d_state, b_state));
  HIP_RETURN(hipMalloc(&m->d_work, b_work));
  HIP_RETURN(hipMalloc(&m->d_window, b_win));
  HIP_RETURN(hipMalloc(&m->d_crops, b_crops));
  HIP_RETURN(hipMalloc(&m->d_jobs, b_jobs));
  m->bytes = b_tri + b_views + b_sv + b_state + b_work + b_win + b_crops + b_jobs;
  HIP_RETURN(hipMemcpy(m->d_tri, triangles, b_tri, hipMemcpyHostToDevice));
  HIP_RETURN(hipMemcpy(m->d_views, table.data(), b_views, hipMemcpyHostToDevice));
  HIP_RETURN(hipMemset(m->d_state, 0, b_state));
  HIP_RETURN(hipMemset(m->d_window, 0, b_win));
  HIP_RETURN(hipMemset(m->d_crops, 0, b_crops));   // no slot has a crop before the first call
  HIP_RETURN(hipMemset(m->d_jobs, 0, b_jobs));
  HIP_RETURN(hipEventCreateWithFlags(&m->done, hipEventDisableTiming));
  return LMX_OK;
}
}  // namespace

extern "C" lmx_status lmx_rough_trace_min(double degrees, double* trace_min) {
  if (!trace_min) { lmx::set_error("lmx_rough_trace_min: null argument"); return LMX_ERR_INVALID_ARG; }
  if (!(degrees > 0.0 && degrees < 180.0)) { lmx::set_error("lmx_rough_trace_min: %g degrees (expected an angle inside (0, 180))", degrees); return LMX_ERR_INVALID_ARG; }
  *trace_min = 1.0 + 2.0 * std::cos(degrees * 3.14159265358979323846 / 180.0);
  return LMX_OK;
}

extern "C" lmx_status lmx_rough_model_create(int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam, const lmx_mesh_view* views,
                                             int32_t n_views, const double* D, const double* ori_dists, int32_t cap_slots, int32_t max_window_w,
                                             int32_t max_window_h, lmx_rough_model** out) {
  return lmx::guarded("lmx_rough_model_create", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_rough_model_create";
    if (!out) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    *out = nullptr;
    mr::Camera dc;
    if (lmx_status st = mesh_check_args(what, triangles, n_triangles, cam, views, n_views, &dc)) return st;
    if (n_views < 1) { set_error("%s: n_views = %d", what, n_views); return LMX_ERR_INVALID_ARG; }
    if (cap_slots < 1 || cap_slots > (1 << 16)) { set_error("%s: cap_slots = %d (1 .. 2^16)", what, cap_slots); return LMX_ERR_INVALID_ARG; }
    if (max_window_w < 1 || max_window_w > dc.W || max_window_h < 1 || max_window_h > dc.H) {
      set_error("%s: a window of %d x %d (1 .. the camera's %d x %d)", what, max_window_w, max_window_h, dc.W, dc.H);
      return LMX_ERR_INVALID_ARG;
    }
    std::vector<rp::View> table((size_t)n_views);
    for (int32_t v = 0; v < n_views; ++v) {
      const double* R = views[v].R;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          const double e = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1.0 : 0.0);   // R^T R - I
          if (!(std::fabs(e) <= 1e-6)) { set_error("%s: view %d is not a rotation (R^T R - I has an entry of %g)", what, v, e); return LMX_ERR_INVALID_ARG; }
        }
      rp::View& t = table[(size_t)v];
      std::memcpy(t.R, R, sizeof(t.R));
      t.distance = views[v].distance;
      t.D = D ? D[v] : 0.0;
      t.ori_dist = ori_dists ? ori_dists[v] : 0.0;
      if (!std::isfinite(t.D) || !std::isfinite(t.ori_dist)) { set_error("%s: view %d has a non-finite D or ori_dist", what, v); return LMX_ERR_INVALID_ARG; }
      rp::quat_of(t.R, t.q);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("%s: device %d of %d", what, device, ndev); return LMX_ERR_INVALID_ARG; }
    lmx_rough_model* m = new lmx_rough_model();
    m->device = device; m->cam = dc; m->n_tri = n_triangles; m->n_views = n_views; m->cap_slots = cap_slots; m->win_w = max_window_w; m->win_h = max_window_h;
    m->win_stride = (size_t)max_window_h * (size_t)dv::crop_pitch(max_window_w);
    const lmx_status st = rough_model_fill(m, triangles, table);
    if (st != LMX_OK) { rough_model_release(m); return st; }
    *out = m;
    return LMX_OK;
  });
}

extern "C" void lmx_rough_model_free(lmx_rough_model* m) {
  if (!m) return;
  if (hipSetDevice(m->device) == hipSuccess) (void)hipDeviceSynchronize();   // a call's kernels may still read the arena
  rough_model_release(m);
}

extern "C" size_t lmx_rough_model_device_bytes(const lmx_rough_model* m) { return m ? m->bytes : 0; }

extern "C" lmx_status lmx_debug_rough_crop(lmx_rough_model* m, int32_t slot, uint16_t* out, int32_t rect[4]) {
  return lmx::guarded("lmx_debug_rough_crop", [&]() -> lmx_status {
    using namespace lmx;
    const char* what = "lmx_debug_rough_crop";
    if (!m || !out || !rect) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
    if (slot < 0 || slot >= m->cap_slots) { set_error("%s: slot %d of %d", what, slot, m->cap_slots); return LMX_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lk(m->m);
    HIP_RETURN(hipSetDevice(m->device));
    HIP_RETURN(hipDeviceSynchronize());
    rp::CropEntry e;
    int32_t st[kMeshStateWords];
    HIP_RETURN(hipMemcpy(&e, m->d_crops + slot, sizeof(e), hipMemcpyDeviceToHost));
    HIP_RETURN(hipMemcpy(st, m->d_state + (size_t)slot * kMeshStateWords, sizeof(st), hipMemcpyDeviceToHost));
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (!e.data || e.w <= 0 || e.h <= 0) return LMX_OK;
    const int32_t sx0 = st[MS_LEVEL + 0], sy0 = st[MS_LEVEL + 1], sw = st[MS_LEVEL + 2] - sx0 + 1, sh = st[MS_LEVEL + 3] - sy0 + 1;
    const int32_t ox = sx0 - st[MS_UNION + 0], oy = sy0 - st[MS_UNION + 1];
    if (sw < 1 || sh < 1 || ox < 0 || oy < 0 || ox + sw > e.w || oy + sh > e.h || e.h > m->win_h || e.pitch > dv::crop_pitch(m->win_w)) {
      set_error("%s: slot %d holds no consistent window", what, slot);
      return LMX_ERR_INVALID_ARG;
    }
    std::vector<uint16_t> win((size_t)e.h * e.pitch);
    HIP_RETURN(hipMemcpy(win.data(), m->d_window + (size_t)slot * m->win_stride, win.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < sh; ++i) std::memcpy(out + (size_t)i * sw, win.data() + (size_t)(oy + i) * e.pitch + ox, (size_t)sw * sizeof(uint16_t));
    rect[0] = sx0; rect[1] = sy0; rect[2] = sw; rect[3] = sh;
    return LMX_OK;
  });
}
