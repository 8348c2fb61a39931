// Depth check of matches against the rendered depth of their templates (include/lmx.h: lmx_depth_templates_*, lmx_depth_diff_matches): the
// depth half of the reference's depth_normal_diff_calc (src/rgbdDetector.cpp:147-282) with the renders made once instead of per match.
// The arithmetic is lmx_depth_verify.hpp; this file is the storage and the parallel shape:
//
//   atlas          every template's depth render cropped to its silhouette box, rows padded with zeros to 16 bytes, every crop 16-byte
//                  aligned, in chunks of device memory (from_mesh: one per render batch, sized to that batch's crops; from_crops: one);
//                  a table entry per template {address, w, h, pitch}
//   k_depth_crop   from_mesh: copies each view's silhouette box out of the batch's depth planes into its chunk, writing the padding
//   k_depth_diff   one 256-lane workgroup per match.  Lanes run along crop rows, one aligned 16-byte vector (8 pixels) each; a crop
//                  narrower than 64 vectors packs several rows into a wave; waves take rows (groups of rows) in turn.  Scene pixels are
//                  read as uint16 under the in-image predicate of lmx_depth_verify.hpp and nowhere else.  Per-lane sums are 64-bit;
//                  wave shuffles, then LDS across the four waves, then one 16-byte store.  No atomics, no workgroup waits for another.
//   k_depth_diff_records   the same walk (depth_diff_walk, shared by both kernels), one workgroup per RAW record of an output slot, against
//                  the scene lmx_depth_templates_upload_scene left on the device: the input of the scored consumer chain (lmx_f2.hip)
//   scene          one pinned staging buffer and one device buffer per object.  lmx_depth_diff_matches stages the frames that have matches
//                  and waits for its results; upload_scene stages all frames, records an event behind their copies and returns
#include <algorithm>
#include <cstring>
#include <memory>

#include "lmx_internal.hpp"
#include "lmx_depth_verify.hpp"
#include "lmx_mesh_raster.hpp"

namespace lmx {
namespace {

struct DepthCrop {          // table entry: 24 bytes per template
  const uint16_t* data;     // [h][pitch], 16-byte aligned; null for an empty crop
  int32_t w, h, pitch, pad;
};
struct DepthJob { int32_t x, y, template_id, frame; };   // frame: index among the frames uploaded for this call
static_assert(sizeof(DepthCrop) == 24 && sizeof(DepthJob) == 16 && sizeof(lmx_depth_diff_t) == 16, "layouts the kernels rely on");

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

// The crop walk of one match at (x, y) against one scene frame, by a whole 256-lane workgroup: both kernels below end in it.  Every lane of
// the workgroup must arrive (it holds a barrier); lane 0 stores the 16-byte result.
__device__ __forceinline__ void depth_diff_walk(const DepthCrop c, int32_t x, int32_t y, const uint16_t* __restrict__ frame, int W, int H,
                                                lmx_depth_diff_t* __restrict__ out) {
  __shared__ unsigned long long s_sum[4];
  __shared__ int s_valid[4], s_templ[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (c.w <= 0 || c.h <= 0) {   // an empty crop: the same for every lane of the workgroup, before any barrier
    if (tid == 0) *reinterpret_cast<int4*>(out) = make_int4(0, 0, 0, 0);
    return;
  }
  const int vpr = c.pitch / dv::kPitchAlign;        // vectors in a row
  const int lanes_per_row = vpr < 64 ? vpr : 64;
  const int rows_per_pass = 64 / lanes_per_row;     // rows a wave takes at once
  const int sub = lane / lanes_per_row, v0 = lane - sub * lanes_per_row;
  dv::Sums a = {0, 0, 0};
  for (int row0 = wave * rows_per_pass; row0 < c.h; row0 += 4 * rows_per_pass) {
    const int i = row0 + sub;
    if (sub >= rows_per_pass || i >= c.h) continue;
    int32_t Y = 0;
    const bool row_in = dv::scene_row(y, i, H, &Y);
    const uint16_t* trow = c.data + (size_t)i * c.pitch;
    const uint16_t* srow = frame + (size_t)Y * W;     // Y = 0 when the row lies outside: never read then
    for (int v = v0; v < vpr; v += lanes_per_row) {
      const uint4 q = load_global_16(trow + v * dv::kPitchAlign);   // past w: the padding, zeros
      const uint32_t word[4] = {q.x, q.y, q.z, q.w};
      dv::add_vector(word, row_in, x, v * dv::kPitchAlign, W, srow, &a);
    }
  }
  unsigned long long sum = a.sum_abs_mm;
  int nv = a.n_valid, nt = a.n_template;
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    nv += __shfl_down(nv, off, 64);
    nt += __shfl_down(nt, off, 64);
  }
  if (lane == 0) { s_sum[wave] = sum; s_valid[wave] = nv; s_templ[wave] = nt; }
  __syncthreads();
  if (tid == 0) {
    sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    nv = s_valid[0] + s_valid[1] + s_valid[2] + s_valid[3];
    nt = s_templ[0] + s_templ[1] + s_templ[2] + s_templ[3];
    *reinterpret_cast<int4*>(out) = make_int4((int)(uint32_t)sum, (int)(uint32_t)(sum >> 32), nv, nt);
  }
}

__global__ __launch_bounds__(256) void k_depth_diff(const DepthCrop* __restrict__ crops, const DepthJob* __restrict__ jobs,
                                                    const uint16_t* __restrict__ scene, int W, int H, lmx_depth_diff_t* __restrict__ out) {
  const DepthJob job = jobs[blockIdx.x];
  depth_diff_walk(crops[job.template_id], job.x, job.y, scene + (size_t)job.frame * H * W, W, H, &out[blockIdx.x]);
}

// One workgroup per RAW record of an output slot (the device consumer chain carries the result through its sorts: lmx_f2.hip, SCORED).  A
// record that is no job -- a template the table does not hold, a frame the scene does not hold, another class -- gets zeros without a look at
// the table or the scene; the three tests are the same for every lane and come before any barrier.
__global__ __launch_bounds__(256) void k_depth_diff_records(const DepthCrop* __restrict__ crops, int32_t count, const lmx_raw_match_t* __restrict__ recs,
                                                            const uint16_t* __restrict__ scene, int32_t n_frames, int W, int H, int32_t class_index,
                                                            lmx_depth_diff_t* __restrict__ diffs) {
  const lmx_raw_match_t r = recs[blockIdx.x];
  if (r.template_id < 0 || r.template_id >= count || r.frame < 0 || r.frame >= n_frames || (class_index >= 0 && r.class_index != class_index)) {
    if (threadIdx.x == 0) *reinterpret_cast<int4*>(&diffs[blockIdx.x]) = make_int4(0, 0, 0, 0);
    return;
  }
  depth_diff_walk(crops[r.template_id], r.x, r.y, scene + (size_t)r.frame * H * W, W, H, &diffs[blockIdx.x]);
}

}  // namespace
}  // namespace lmx

#define DV_HIP(expr)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      lmx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
      return e_ == hipErrorNoDevice ? LMX_ERR_NO_DEVICE : LMX_ERR_HIP;                             \
    }                                                                                              \
  } while (0)

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
  bool scene_pending = false;            // scene_ready has been recorded and h_scene may still be read by a copy
  lmx::DepthJob *d_jobs = nullptr, *h_jobs = nullptr;
  lmx_depth_diff_t *d_out = nullptr, *h_out = nullptr;
  size_t jobs_cap = 0;                   // entries
  std::vector<uint32_t> sel;             // scratch of a call: the matches it computes
  std::vector<int32_t> sel_slot;         // scratch of a call: the uploaded frame of each of them
  std::vector<int32_t> slot;             // scratch of a call: frame -> uploaded frame, or -1

  lmx_status ensure_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { lmx::set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
    DV_HIP(hipSetDevice(device));
    if (!s) DV_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (!scene_ready) DV_HIP(hipEventCreateWithFlags(&scene_ready, hipEventDisableTiming));
    if (!d_table && !table.empty()) {
      DV_HIP(hipMalloc(&d_table, table.size() * sizeof(lmx::DepthCrop)));
      DV_HIP(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(lmx::DepthCrop), hipMemcpyHostToDevice, s));
      DV_HIP(hipStreamSynchronize(s));
    }
    return LMX_OK;
  }
  // The staging buffer is free again: the copies of the previous upload_scene have left it.
  lmx_status wait_scene_copies() {
    if (scene_pending) { DV_HIP(hipEventSynchronize(scene_ready)); scene_pending = false; }
    return LMX_OK;
  }
  // A call failed with copies of earlier frames possibly still queued: nothing may read the staging buffer once the call has returned, since
  // no event stands behind those copies for the next call to wait on.  The error already set is the one reported.
  void drain_after_error() { (void)hipStreamSynchronize(s); }
  lmx_status grow_scene(size_t bytes) {
    if (bytes <= scene_cap) return LMX_OK;
    DV_HIP(hipStreamSynchronize(s));     // nothing queued may still use the buffers that go
    (void)hipFree(d_scene); (void)hipHostFree(h_scene);
    d_scene = h_scene = nullptr; scene_cap = 0;
    const size_t cap = bytes;
    DV_HIP(hipMalloc(&d_scene, cap));
    DV_HIP(hipHostMalloc(&h_scene, cap, hipHostMallocDefault));
    scene_cap = cap;
    return LMX_OK;
  }
  lmx_status grow_jobs(size_t n) {
    if (n <= jobs_cap) return LMX_OK;
    (void)hipFree(d_jobs); (void)hipFree(d_out); (void)hipHostFree(h_jobs); (void)hipHostFree(h_out);
    d_jobs = h_jobs = nullptr; d_out = h_out = nullptr; jobs_cap = 0;
    const size_t cap = std::max(n, (size_t)1024);
    DV_HIP(hipMalloc(&d_jobs, cap * sizeof(lmx::DepthJob)));
    DV_HIP(hipMalloc(&d_out, cap * sizeof(lmx_depth_diff_t)));
    DV_HIP(hipHostMalloc(&h_jobs, cap * sizeof(lmx::DepthJob), hipHostMallocDefault));
    DV_HIP(hipHostMalloc(&h_out, cap * sizeof(lmx_depth_diff_t), hipHostMallocDefault));
    jobs_cap = cap;
    return LMX_OK;
  }
  void add(const uint16_t* data, int32_t w, int32_t h, const int32_t rect[4]) {
    table.push_back(lmx::DepthCrop{data, w, h, w > 0 ? lmx::dv::crop_pitch(w) : 0, 0});
    rects.insert(rects.end(), rect, rect + 4);
  }
  ~lmx_depth_templates() {
    if (s) (void)hipStreamSynchronize(s);
    for (void* p : chunks) (void)hipFree(p);
    (void)hipFree(d_table); (void)hipFree(d_scene); (void)hipFree(d_jobs); (void)hipFree(d_out);
    (void)hipHostFree(h_scene); (void)hipHostFree(h_jobs); (void)hipHostFree(h_out);
    if (scene_ready) (void)hipEventDestroy(scene_ready);
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
    DV_HIP(hipMalloc(&d_tri.p, (size_t)n_triangles * 9 * sizeof(double)));
    DV_HIP(hipMalloc(&d_views.p, (size_t)B * 10 * sizeof(double)));
    DV_HIP(hipMalloc(&d_work.p, (size_t)B * n_triangles * sizeof(mr::Tri)));
    DV_HIP(hipMalloc(&d_state.p, state.size() * 4));
    DV_HIP(hipMalloc(&d_depth.p, px * B * sizeof(uint16_t)));
    DV_HIP(hipMemcpyAsync(d_tri.p, triangles, (size_t)n_triangles * 9 * sizeof(double), hipMemcpyHostToDevice, s));
    for (int first = 0; first < n_views; first += B) {
      const int n = std::min(B, n_views - first);
      DV_HIP(hipMemcpyAsync(d_views.p, views + first, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice, s));
      launch_mesh_raster(s, d_tri.as<double>(), n_triangles, dc, d_views.as<double>(), n, 1, d_work.as<mr::Tri>(), d_state.as<int32_t>(), nullptr,
                         d_depth.as<uint16_t>(), nullptr);
      DV_HIP(hipGetLastError());
      DV_HIP(hipMemcpyAsync(state.data(), d_state.p, (size_t)n * kMeshStateWords * 4, hipMemcpyDeviceToHost, s));
      DV_HIP(hipStreamSynchronize(s));
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
        DV_HIP(hipMalloc(&chunk, elems * sizeof(uint16_t)));
        t->chunks.push_back(chunk);
        t->atlas_bytes += elems * sizeof(uint16_t);
        hipLaunchKernelGGL(k_depth_crop, dim3(16, (unsigned)n), dim3(256), 0, s, d_depth.as<uint16_t>(), d_state.as<int32_t>(), dc.W, dc.H, chunk, where);
        DV_HIP(hipGetLastError());
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
    DV_HIP(hipStreamSynchronize(s));   // the scratch buffers go when this returns
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
      DV_HIP(hipMalloc(&chunk, bytes));
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
      DV_HIP(hipMemcpyAsync(chunk, packed.data(), bytes, hipMemcpyHostToDevice, t->s));
      DV_HIP(hipStreamSynchronize(t->s));
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
    DV_HIP(hipMemcpy2DAsync(out, (size_t)c.w * 2, c.data, (size_t)c.pitch * 2, (size_t)c.w * 2, (size_t)c.h, hipMemcpyDeviceToHost, t->s));
    DV_HIP(hipStreamSynchronize(t->s));
    return LMX_OK;
  });
}

extern "C" size_t lmx_depth_templates_device_bytes(const lmx_depth_templates* t) {
  return t ? t->atlas_bytes + t->table.size() * sizeof(lmx::DepthCrop) : 0;
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
  DV_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t*>(t->d_scene) + frame_bytes * slot, h, frame_bytes, hipMemcpyHostToDevice, t->s));
  return LMX_OK;
}

// The device half of a depth check on the host's match list: the first n entries of h_jobs against the W x H frames already in d_scene
// (a job's frame is its slot there): job upload, k_depth_diff, read-back into h_out.  The object's mutex is the caller's to hold.
lmx_status run_jobs(lmx_depth_templates* t, size_t n, int32_t W, int32_t H) {
  hipStream_t s = t->s;
  DV_HIP(hipMemcpyAsync(t->d_jobs, t->h_jobs, n * sizeof(lmx::DepthJob), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(lmx::k_depth_diff, dim3((unsigned)n), dim3(256), 0, s, t->d_table, t->d_jobs, t->d_scene, W, H, t->d_out);
  DV_HIP(hipGetLastError());
  DV_HIP(hipMemcpyAsync(t->h_out, t->d_out, n * sizeof(lmx_depth_diff_t), hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
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

namespace lmx {

std::mutex& depth_templates_mutex(lmx_depth_templates* t) { return t->m; }

DepthSceneInfo depth_templates_scene(const lmx_depth_templates* t) {
  return DepthSceneInfo{t->device, (int32_t)t->table.size(), t->scene_frames, t->scene_W, t->scene_H};
}

lmx_status depth_upload_scene(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames) {
  if (n_frames < 1) { set_error("lmx_depth_templates_upload_scene: n_frames = %d", n_frames); return LMX_ERR_INVALID_ARG; }
  if (lmx_status st = check_depth_frames("lmx_depth_templates_upload_scene", depth, n_frames)) return st;
  const int32_t W = depth[0].cols, H = depth[0].rows;
  if (lmx_status st = t->ensure_device()) return st;
  if (lmx_status st = t->wait_scene_copies()) return st;   // the previous scene's copies still read the staging buffer
  t->scene_frames = 0;
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

lmx_status depth_launch_records(lmx_depth_templates* t, hipStream_t s, const lmx_raw_match_t* d_recs, uint32_t n_records, int32_t class_index,
                                lmx_depth_diff_t* d_diffs) {
  if (t->scene_frames < 1) { set_error("no scene uploaded: call lmx_depth_templates_upload_scene first"); return LMX_ERR_INVALID_ARG; }
  DV_HIP(hipStreamWaitEvent(s, t->scene_ready, 0));
  if (n_records == 0) return LMX_OK;
  hipLaunchKernelGGL(k_depth_diff_records, dim3(n_records), dim3(256), 0, s, t->d_table, (int32_t)t->table.size(), d_recs, t->d_scene, t->scene_frames,
                     t->scene_W, t->scene_H, class_index, d_diffs);
  DV_HIP(hipGetLastError());
  return LMX_OK;
}

lmx_status depth_diff_resident(lmx_depth_templates* t, const lmx_match_t* matches, size_t n, int32_t frame, int32_t class_index, lmx_depth_diff_t* out) {
  if (n == 0) return LMX_OK;
  if (frame < 0 || frame >= t->scene_frames) { set_error("frame %d is not in the uploaded scene (%d frames)", frame, t->scene_frames); return LMX_ERR_INVALID_ARG; }
  if (n > 0x7fffffffull) { set_error("%zu matches in one frame", n); return LMX_ERR_INVALID_ARG; }
  std::memset(out, 0, n * sizeof(lmx_depth_diff_t));
  const size_t count = t->table.size();
  t->sel.clear();
  for (size_t i = 0; i < n; ++i) {
    const lmx_match_t& m = matches[i];
    if (class_index >= 0 && m.class_index != class_index) continue;
    if (m.template_id < 0 || (size_t)m.template_id >= count) continue;   // zeros, as k_depth_diff_records gives; the cluster step refuses the id
    t->sel.push_back((uint32_t)i);
  }
  const size_t n_sel = t->sel.size();
  if (n_sel == 0) return LMX_OK;
  if (lmx_status st = t->grow_jobs(n_sel)) return st;
  for (size_t k = 0; k < n_sel; ++k) {
    const lmx_match_t& m = matches[t->sel[k]];
    t->h_jobs[k] = DepthJob{m.x, m.y, m.template_id, frame};
  }
  if (lmx_status st = run_jobs(t, n_sel, t->scene_W, t->scene_H)) return st;   // on the object's stream, behind the scene's copies
  for (size_t k = 0; k < n_sel; ++k) out[t->sel[k]] = t->h_out[k];
  return LMX_OK;
}

}  // namespace lmx

extern "C" lmx_status lmx_depth_diff_matches(lmx_depth_templates* t, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                                             const size_t* offsets, int32_t class_index, lmx_depth_diff_t* out) {
  return lmx::guarded("lmx_depth_diff_matches", [&]() -> lmx_status {
    using namespace lmx;
    if (!t) { set_error("lmx_depth_diff_matches: null argument"); return LMX_ERR_INVALID_ARG; }
    if (n_frames < 0) { set_error("lmx_depth_diff_matches: n_frames = %d", n_frames); return LMX_ERR_INVALID_ARG; }
    if (n_frames == 0) return LMX_OK;
    if (!depth || !offsets) { set_error("lmx_depth_diff_matches: null argument"); return LMX_ERR_INVALID_ARG; }
    if (offsets[0] != 0) { set_error("lmx_depth_diff_matches: offsets[0] = %zu (expected 0)", offsets[0]); return LMX_ERR_INVALID_ARG; }
    for (int32_t f = 0; f < n_frames; ++f)
      if (offsets[f + 1] < offsets[f]) { set_error("lmx_depth_diff_matches: offsets[%d] = %zu is below offsets[%d] = %zu", f + 1, offsets[f + 1], f, offsets[f]); return LMX_ERR_INVALID_ARG; }
    if (lmx_status st = check_depth_frames("lmx_depth_diff_matches", depth, n_frames)) return st;
    const int32_t W = depth[0].cols, H = depth[0].rows;
    const size_t n_matches = offsets[n_frames];
    if (n_matches == 0) return LMX_OK;
    if (!matches || !out) { set_error("lmx_depth_diff_matches: null argument"); return LMX_ERR_INVALID_ARG; }
    if (n_matches > 0x7fffffffull) { set_error("lmx_depth_diff_matches: %zu matches in one call", n_matches); return LMX_ERR_INVALID_ARG; }   // sel holds uint32, the grid is n_sel wide
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
        if (m.template_id < 0 || (size_t)m.template_id >= count) { set_error("lmx_depth_diff_matches: match %zu: template_id %d outside [0, %zu)", i, m.template_id, count); return LMX_ERR_INVALID_ARG; }
        if (t->slot[f] < 0) t->slot[f] = n_slots++;
        t->sel.push_back((uint32_t)i);
        t->sel_slot.push_back(t->slot[f]);
      }
    std::memset(out, 0, n_matches * sizeof(lmx_depth_diff_t));
    const size_t n_sel = t->sel.size();
    if (n_sel == 0) return LMX_OK;
    if (lmx_status st = t->ensure_device()) return st;
    const size_t frame_bytes = (size_t)W * H * sizeof(uint16_t);
    // the frames that have matches take the place of an uploaded scene: staged row by row into pinned memory, each on its way while the
    // next is staged
    if (lmx_status st = t->wait_scene_copies()) return st;
    t->scene_frames = 0;
    if (lmx_status st = t->grow_scene(frame_bytes * n_slots)) return st;
    if (lmx_status st = t->grow_jobs(n_sel)) return st;
    for (int32_t f = 0; f < n_frames; ++f)
      if (t->slot[f] >= 0)
        if (lmx_status st = queue_frame(t, depth[f], t->slot[f], W, H)) { t->drain_after_error(); return st; }
    for (size_t k = 0; k < n_sel; ++k) {
      const lmx_match_t& m = matches[t->sel[k]];
      t->h_jobs[k] = DepthJob{m.x, m.y, m.template_id, t->sel_slot[k]};
    }
    if (lmx_status st = run_jobs(t, n_sel, W, H)) { t->drain_after_error(); return st; }
    for (size_t k = 0; k < n_sel; ++k) out[t->sel[k]] = t->h_out[k];
    return LMX_OK;
  });
}
