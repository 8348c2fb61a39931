// Trainer side of the bank: cv::linemod::Detector::addTemplate as the reference's trainers call it
// (/root/reference/src/renderer.cpp:308, src/renderer_only_image.cpp:266).
//
// Device: the per-pixel stages -- quantizedOrientations (+ squared magnitudes), quantizedNormals + medianBlur, the pyrDown /
// nearest-neighbour chains -- with the same kernels match() uses (no size constraint: linearize is not part of training).
// Host: extractTemplate's candidate ranking and the greedy scattered selection, cropTemplates.  Those are short sequential
// loops over a few thousand candidates with a data-dependent restart rule; they stay on the CPU like upstream.

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lmx_internal.hpp"
#include "lmx_mesh_raster.hpp"
#include "lmx_train_cand.hpp"
#include "lmx_train_select.hpp"

namespace lmx {
namespace {

#define TR_HIP(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return e_ == hipErrorNoDevice ? LMX_ERR_NO_DEVICE : LMX_ERR_HIP;                     \
    }                                                                                      \
  } while (0)

using namespace train_select;

std::vector<Modality> select_modalities(const lmx_bank* bank) {
  std::vector<Modality> mods;
  for (const lmx_modality_desc& md : bank->mods) mods.push_back(Modality{md.type == LMX_MOD_COLOR_GRADIENT, md.num_features, md.strong_threshold, md.extract_threshold});
  return mods;
}

}  // namespace

lmx_status train_add_template(lmx_bank* bank, int device, const lmx_image* sources, int n_sources, const char* class_id,
                              const lmx_image* object_mask, int32_t* template_id, int32_t* bounding_box) {
  const int L = (int)bank->T.size(), M = (int)bank->mods.size();
  if (n_sources != M) { set_error("sources.size()=%d != modalities.size()=%d", n_sources, M); return LMX_ERR_SHAPE; }
  const int H0 = sources[0].rows, W0 = sources[0].cols;
  if (H0 < 16 || W0 < 16) { set_error("source image too small"); return LMX_ERR_SHAPE; }
  const std::vector<Modality> sel_mods = select_modalities(bank);
  { std::string why; if (!check_num_features(sel_mods, L, &why)) { set_error("lmx_bank_add_template: %s", why.c_str()); return LMX_ERR_SHAPE; } }
  // ColorGradient sources are 8UC3, or 8UC1 (a gray image: the one-plane quantiser, whose templates equal those of the image copied into
  // B, G and R)
  for (int m = 0; m < M; ++m) {
    const bool cg = bank->mods[m].type == LMX_MOD_COLOR_GRADIENT;
    const lmx_image& im = sources[m];
    const bool ch_ok = cg ? (im.channels == 3 || im.channels == 1) : im.channels == 1;
    if (!im.data || im.rows != H0 || im.cols != W0 || !ch_ok || im.elem_size != (cg ? 1 : 2) ||
        im.row_stride_bytes < (size_t)W0 * (cg ? im.channels : 2)) {
      set_error("source %d: expected %s of size %dx%d", m, cg ? "8UC3 or 8UC1" : "16UC1", W0, H0);
      return LMX_ERR_SHAPE;
    }
  }
  std::vector<std::vector<uint8_t>> masks(L);  // per level (INTER_NEAREST /2 per pyrDown); empty = no mask
  if (object_mask && object_mask->data) {
    if (object_mask->rows != H0 || object_mask->cols != W0 || object_mask->channels != 1 || object_mask->elem_size != 1) {
      set_error("object_mask must be 8UC1 of the source size");
      return LMX_ERR_SHAPE;
    }
    masks[0].resize((size_t)H0 * W0);
    for (int y = 0; y < H0; ++y)
      std::memcpy(&masks[0][(size_t)y * W0], (const uint8_t*)object_mask->data + (size_t)y * object_mask->row_stride_bytes, (size_t)W0);
    for (int l = 1, h = H0, w = W0; l < L; ++l) {
      const int hn = h / 2, wn = w / 2;
      masks[l].resize((size_t)hn * wn);
      for (int y = 0; y < hn; ++y)
        for (int x = 0; x < wn; ++x) masks[l][(size_t)y * wn + x] = masks[l - 1][(size_t)(2 * y) * w + 2 * x];
      h = hn; w = wn;
    }
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  TR_HIP(hipSetDevice(device));

  // ---- device: labels (+ magnitudes) per modality and level -------------------------------------------------------------
  std::vector<std::vector<std::vector<uint8_t>>> labels(M, std::vector<std::vector<uint8_t>>(L));
  std::vector<std::vector<std::vector<float>>> mags(M, std::vector<std::vector<float>>(L));
  std::vector<void*> to_free;
  auto cleanup = [&]() { for (void* p : to_free) (void)hipFree(p); to_free.clear(); };
  auto dmalloc = [&](size_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, std::max<size_t>(bytes, 256) + 64) != hipSuccess) return nullptr; to_free.push_back(p); return p; };
  lmx_status st = LMX_OK;
  auto run = [&]() -> lmx_status {
    for (int m = 0; m < M; ++m) {
      const lmx_modality_desc& md = bank->mods[m];
      const bool cg = md.type == LMX_MOD_COLOR_GRADIENT;
      const int px_bytes = cg ? sources[m].channels : 2;   // colour: 3 (BGR) or 1 (gray)
      const size_t px0 = (size_t)H0 * W0, row_bytes = (size_t)W0 * px_bytes;
      std::vector<uint8_t> packed(px0 * px_bytes);
      for (int y = 0; y < H0; ++y) std::memcpy(&packed[(size_t)y * row_bytes], (const uint8_t*)sources[m].data + (size_t)y * sources[m].row_stride_bytes, row_bytes);
      void* d_src = dmalloc(packed.size());
      if (!d_src) { set_error("hipMalloc failed"); return LMX_ERR_HIP; }
      TR_HIP(hipMemcpy(d_src, packed.data(), packed.size(), hipMemcpyHostToDevice));
      uint8_t* d_prev_q = nullptr;
      uint8_t* d_cur_src = (uint8_t*)d_src;
      int h = H0, w = W0;
      for (int l = 0; l < L; ++l) {
        const int prev_h = h, prev_w = w;
        if (l > 0) { h /= 2; w /= 2; }
        if (h < 1 || w < 1) { set_error("image too small for %d pyramid levels", L); return LMX_ERR_SHAPE; }
        uint8_t* d_q = (uint8_t*)dmalloc((size_t)h * w);
        if (!d_q) { set_error("hipMalloc failed"); return LMX_ERR_HIP; }
        labels[m][l].resize((size_t)h * w);
        if (cg) {
          float* d_mag = (float*)dmalloc((size_t)h * w * 4);
          uint8_t* d_next = l + 1 < L ? (uint8_t*)dmalloc((size_t)(h / 2) * (w / 2) * px_bytes) : nullptr;
          if (!d_mag || (l + 1 < L && !d_next)) { set_error("hipMalloc failed"); return LMX_ERR_HIP; }
          launch_color_quantize(nullptr, d_cur_src, d_q, d_next, h, w, 1, md.weak_threshold, d_mag, nullptr, nullptr, px_bytes, 0);
          TR_HIP(hipDeviceSynchronize());
          mags[m][l].resize((size_t)h * w);
          TR_HIP(hipMemcpy(mags[m][l].data(), d_mag, (size_t)h * w * 4, hipMemcpyDeviceToHost));
          d_cur_src = d_next;
        } else {
          if (l == 0) {
            std::vector<uint8_t> bins;
            if (!normal_bins_device_image(bank->normal_lut.data(), bins)) { set_error("bank holds an invalid normal LUT"); return LMX_ERR_INVALID_ARG; }
            uint8_t* d_bins = (uint8_t*)dmalloc(bins.size());
            if (!d_bins) { set_error("hipMalloc failed"); return LMX_ERR_HIP; }
            TR_HIP(hipMemcpy(d_bins, bins.data(), bins.size(), hipMemcpyHostToDevice));
            launch_depth_quantize(nullptr, (const uint16_t*)d_src, d_q, nullptr, h, w, 1, md.distance_threshold, md.difference_threshold, d_bins);
          }
          else launch_nn_down2(nullptr, d_prev_q, d_q, prev_h, prev_w, h, w, 1);
          TR_HIP(hipDeviceSynchronize());
        }
        TR_HIP(hipMemcpy(labels[m][l].data(), d_q, (size_t)h * w, hipMemcpyDeviceToHost));
        d_prev_q = d_q;
      }
    }
    return LMX_OK;
  };
  st = run();
  cleanup();
  if (st != LMX_OK) return st;

  // ---- host: extractTemplate per (level, modality) on each level's window, cropTemplates (lmx_train_select.hpp) -----------------------
  *template_id = -1;
  std::vector<LevelArrays> levels(L);
  for (int l = 0, h = H0, w = W0; l < L; ++l) {
    if (l > 0) { h /= 2; w /= 2; }
    LevelArrays& lv = levels[l];
    lv.w = w; lv.h = h;
    lv.mask = masks[l].empty() ? nullptr : masks[l].data();
    for (int m = 0; m < M; ++m) {
      lv.label.push_back(labels[m][l].data());
      lv.mag.push_back(mags[m][l].empty() ? nullptr : mags[m][l].data());
    }
  }
  Pyramid pyr;
  std::string why;
  const Status sel = select_pyramid(levels, sel_mods, &pyr, &why);
  if (sel == BAD_ARGUMENT) { set_error("lmx_bank_add_template: %s", why.c_str()); return LMX_ERR_SHAPE; }
  if (sel == REJECTED) return LMX_OK;  // upstream: addTemplate returns -1, nothing is added
  const std::vector<int32_t>& templates = pyr.templates;
  const std::vector<int32_t>& features = pyr.features;
  const int32_t fb = (int32_t)(features.size() / 3);
  const int32_t existing = lmx_bank_num_templates(bank, class_id);
  st = lmx_bank_add_class(bank, class_id, 1, templates.data(), features.data(), fb);
  if (st != LMX_OK) return st;
  *template_id = existing;
  if (bounding_box) std::memcpy(bounding_box, pyr.bounding_box, sizeof(pyr.bounding_box));
  return LMX_OK;
}


// ---- batched trainer over rendered views (lmx_bank_train_mesh) -------------------------------------------------------------------------
// The trainer loop of the reference (src/renderer.cpp:262-329) with the renderer and the per-pixel half of addTemplate on the device, B views
// per pass: k_mesh_* render gray / depth / mask into device memory, the quantisers run with n_frames = B (the gray render through the
// one-plane colour quantiser), k_mesh_pack writes each view's windows (silhouette box grown by 2, per level: the same window
// train_add_template derives on the host) of magnitudes, labels and mask into a pinned host buffer.  One stream, one synchronisation per
// batch; the host half (select_pyramid of lmx_train_select.hpp) runs on a few threads,
// one view each, while the device works on the next batch.  Templates are appended to the bank in view order when every batch is done.
// With device candidates (lmx_bank_train_mesh_opts) k_train_candidates takes k_mesh_pack's place: per (view, level, modality) it leaves the
// window's candidate list (lmx_train_cand.hpp) and only the lists are read back; the host half is then select_view_from_lists -- decode,
// rank, select, crop.  Views whose lists carry a status are rendered again in a second pass through the packed read-back.
namespace {

constexpr int kMeshTrainBatch = 32;   // views per pass: 32 x ~100 covered tiles fill the 256 CUs; two pinned read-back buffers of 32 worst-case slots
constexpr int kMeshTrainThreads = 8;  // host selection threads: a fixed small pool, never sized by the machine (LMX_TRAIN_THREADS = 1 .. 16 overrides)

struct ViewResult {
  bool accepted = false;
  lmx_status status = LMX_OK;
  std::string error;
  std::vector<int32_t> templates, features;   // [L*M][5] with feat_begin relative to this view, [n][3]
};

// extractTemplate per (modality, level) on one view's packed windows, then cropTemplates: the host half of train_add_template
void select_view(const lmx_bank* bank, const uint8_t* slot, const int32_t* state, int W0, int H0, ViewResult& out) {
  const int L = (int)bank->T.size(), M = (int)bank->mods.size();
  int n_cg = 0;
  for (int m = 0; m < M; ++m) n_cg += bank->mods[m].type == LMX_MOD_COLOR_GRADIENT;
  std::vector<LevelArrays> levels(L);
  size_t off = 0;
  for (int l = 0; l < L; ++l) {
    LevelArrays& lv = levels[l];
    mesh_window(state + MS_LEVEL + 4 * l, W0 >> l, H0 >> l, &lv.x0, &lv.y0, &lv.w, &lv.h);
    const size_t n = (size_t)lv.w * lv.h;
    const uint8_t* base = slot + off;
    for (int m = 0, cg_index = 0; m < M; ++m) {
      const bool cg = bank->mods[m].type == LMX_MOD_COLOR_GRADIENT;
      lv.label.push_back(base + n * 4 * n_cg + n * m);
      lv.mag.push_back(cg ? reinterpret_cast<const float*>(base + n * 4 * cg_index) : nullptr);
      cg_index += cg;
    }
    lv.mask = base + n * 4 * n_cg + n * M;
    off += mesh_pack_level_bytes(lv.w, lv.h, M, n_cg);
  }
  Pyramid pyr;
  const Status sel = select_pyramid(levels, select_modalities(bank), &pyr, &out.error);
  if (sel == BAD_ARGUMENT) { out.status = LMX_ERR_SHAPE; return; }
  if (sel == REJECTED) return;   // upstream: addTemplate returns -1, nothing is added
  out.templates.swap(pyr.templates);
  out.features.swap(pyr.features);
  out.accepted = true;
}

// The same from the device's candidate lists (lmx_train_cand.hpp; hd = the view's [L][M] headers, recs = the batch's records): decode each
// list, shift it by its window's origin, rank and select (select_from_list), cropTemplates.  -> false: a list carries a status (window too
// large for the kernel, record buffer full) and the view must go through the pack-and-host path; nothing of `out` is set then.
bool select_view_from_lists(const lmx_bank* bank, const train_cand::ListHeader* hd, const train_cand::Record* recs, uint32_t cap, const int32_t* state, int W0,
                            int H0, ViewResult& out) {
  const int L = (int)bank->T.size(), M = (int)bank->mods.size();
  for (int k = 0; k < L * M; ++k) {
    if (hd[k].status) return false;
    if ((uint64_t)hd[k].offset + hd[k].n_cands > (uint64_t)cap) throw std::runtime_error("candidate list outside the record buffer");
  }
  const std::vector<Modality> mods = select_modalities(bank);
  std::vector<std::vector<Feat>> tp((size_t)L * M);
  for (int m = 0; m < M; ++m) {
    size_t num_features = (size_t)mods[m].num_features;
    for (int l = 0; l < L; ++l) {
      if (l > 0) num_features /= 2;
      int x0, y0, w, h;
      mesh_window(state + MS_LEVEL + 4 * l, W0 >> l, H0 >> l, &x0, &y0, &w, &h);
      const train_cand::ListHeader& lh = hd[(size_t)l * M + m];
      if (!select_from_list(mods[m].color, lh, recs + lh.offset, x0, y0, num_features, tp[(size_t)l * M + m])) return true;   // rejected
    }
  }
  Pyramid pyr;
  crop_templates(tp, M, &pyr);
  out.templates.swap(pyr.templates);
  out.features.swap(pyr.features);
  out.accepted = true;
  return true;
}

struct MeshTrainBuffers {   // everything a call allocates: freed in one place
  std::vector<void*> dev, pinned;
  hipStream_t stream = nullptr;
  ~MeshTrainBuffers() {
    if (stream) { (void)hipStreamSynchronize(stream); }
    for (void* p : dev) (void)hipFree(p);
    for (void* p : pinned) (void)hipHostFree(p);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

}  // namespace

lmx_status train_mesh(lmx_bank* bank, int device, const double* triangles, int n_tri, const lmx_mesh_camera* cam, const mr::Camera& dc,
                      const lmx_mesh_view* views, int n_views, const char* class_id, int32_t* template_ids, lmx_renderer_params** side_car,
                      bool device_candidates, lmx_train_mesh_stats* stats) {
  const int L = (int)bank->T.size(), M = (int)bank->mods.size();
  const int W0 = dc.W, H0 = dc.H;
  if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->n_views = n_views; }
  if (H0 < 16 || W0 < 16) { set_error("source image too small"); return LMX_ERR_SHAPE; }
  if (L < 1 || L > kMaxLevels || M < 1 || M > kMaxModalities) { set_error("lmx_bank_train_mesh: %d pyramid levels x %d modalities are not supported", L, M); return LMX_ERR_SHAPE; }
  if ((H0 >> (L - 1)) < 1 || (W0 >> (L - 1)) < 1) { set_error("image too small for %d pyramid levels", L); return LMX_ERR_SHAPE; }
  { std::string why; if (!check_num_features(select_modalities(bank), L, &why)) { set_error("lmx_bank_train_mesh: %s", why.c_str()); return LMX_ERR_SHAPE; } }
  int n_cg = 0;
  bool any_dn = false;
  for (int m = 0; m < M; ++m) {
    if (bank->mods[m].type == LMX_MOD_COLOR_GRADIENT) ++n_cg;
    else if (bank->mods[m].type == LMX_MOD_DEPTH_NORMAL) any_dn = true;
    else { set_error("lmx_bank_train_mesh: unknown modality type %d", bank->mods[m].type); return LMX_ERR_INVALID_ARG; }
  }
  // side-car of the accepted views, filled as we go and handed over at the end
  std::unique_ptr<lmx_renderer_params, void (*)(lmx_renderer_params*)> side(nullptr, lmx_renderer_params_free);
  if (side_car) {
    *side_car = nullptr;
    side.reset(new lmx_renderer_params());
    std::memset(side.get(), 0, sizeof(lmx_renderer_params));
    side->renderer_width = W0; side->renderer_height = H0;
    side->renderer_focal_length_x = cam->fx; side->renderer_focal_length_y = cam->fy;
  }
  if (n_views == 0) { if (side_car) *side_car = side.release(); return LMX_OK; }
  const int bad = mesh_first_invalid_view(triangles, n_tri, views, n_views);
  if (bad >= 0) { set_error("lmx_bank_train_mesh: view %d puts a vertex at or behind the camera (Z <= 0.01); nothing was added", bad); return LMX_ERR_INVALID_ARG; }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  TR_HIP(hipSetDevice(device));
  MeshTrainBuffers buf;
  TR_HIP(hipStreamCreateWithFlags(&buf.stream, hipStreamNonBlocking));
  hipStream_t s = buf.stream;
  // a view's slot in the packed read-back must hold whole levels (worst case); large frames take fewer views per pass so that the two
  // pinned buffers stay below ~2 x 192 MB (640x480 RGB-D: 2.7 MB per slot, the full batch)
  size_t slot_bytes = 0;
  for (int l = 0; l < L; ++l) slot_bytes += mesh_pack_level_bytes(W0 >> l, H0 >> l, M, n_cg);
  slot_bytes = (slot_bytes + 255) & ~(size_t)255;
  const int fit = (int)std::max<size_t>(4, ((size_t)192 << 20) / slot_bytes);
  const int B = std::min(n_views, std::min(kMeshTrainBatch, fit));
  const size_t px0 = (size_t)W0 * H0;
  size_t device_bytes = 0;
  auto dmalloc = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(bytes, 256) + 64) != hipSuccess) return nullptr;
    buf.dev.push_back(p); device_bytes += std::max<size_t>(bytes, 256) + 64;
    return p;
  };
#define TM_ALLOC(var, type, bytes) type var = (type)dmalloc(bytes); if (!var) { set_error("hipMalloc of %zu bytes failed", (size_t)(bytes)); return LMX_ERR_HIP; }
  TM_ALLOC(d_tri, double*, (size_t)n_tri * 9 * sizeof(double));
  TM_ALLOC(d_views, double*, (size_t)B * 10 * sizeof(double));
  TM_ALLOC(d_work, mr::Tri*, (size_t)B * n_tri * sizeof(mr::Tri));
  TM_ALLOC(d_state, int32_t*, (size_t)B * kMeshStateWords * 4);
  TM_ALLOC(d_mask, uint8_t*, px0 * B);
  uint8_t* d_gray = nullptr;
  uint16_t* d_depth = nullptr;
  uint8_t* d_bins = nullptr;
  if (n_cg) { d_gray = (uint8_t*)dmalloc(px0 * B); if (!d_gray) { set_error("hipMalloc failed"); return LMX_ERR_HIP; } }
  if (any_dn) {
    d_depth = (uint16_t*)dmalloc(px0 * B * 2);
    d_bins = (uint8_t*)dmalloc(kNormalBinsDeviceBytes);
    if (!d_depth || !d_bins) { set_error("hipMalloc failed"); return LMX_ERR_HIP; }
    std::vector<uint8_t> bins;
    if (!normal_bins_device_image(bank->normal_lut.data(), bins)) { set_error("bank holds an invalid normal LUT"); return LMX_ERR_INVALID_ARG; }
    TR_HIP(hipMemcpy(d_bins, bins.data(), bins.size(), hipMemcpyHostToDevice));
  }
  TR_HIP(hipMemcpy(d_tri, triangles, (size_t)n_tri * 9 * sizeof(double), hipMemcpyHostToDevice));
  // label images (+ magnitudes, + the one-plane pyrDown chain) per modality and level; a DepthNormal modality keeps level 0 only (its
  // coarser levels are level 0 sub-sampled, which k_mesh_pack reads directly)
  MeshPackArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  uint8_t* d_pyr[kMaxModalities][kMaxLevels] = {};
  for (int l = 0; l < L; ++l) {
    const size_t pxl = (size_t)(W0 >> l) * (H0 >> l);
    for (int m = 0; m < M; ++m) {
      const bool cg = bank->mods[m].type == LMX_MOD_COLOR_GRADIENT;
      if (!cg && l > 0) continue;
      void* q = dmalloc(pxl * B);
      void* mg = cg ? dmalloc(pxl * B * 4) : nullptr;
      void* py = (cg && l > 0) ? dmalloc(pxl * B) : nullptr;
      if (!q || (cg && !mg) || (cg && l > 0 && !py)) { set_error("hipMalloc failed"); return LMX_ERR_HIP; }
      pa.quant[l][m] = (const uint8_t*)q; pa.mag[l][m] = (const float*)mg; d_pyr[m][l] = (uint8_t*)py;
    }
  }
  uint8_t* h_pack[2] = {nullptr, nullptr};
  int32_t* h_state[2] = {nullptr, nullptr};
  size_t pinned_bytes = 0;
  auto pinned = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc of %zu bytes failed", bytes); return nullptr; }
    buf.pinned.push_back(p); pinned_bytes += bytes;
    return p;
  };
  // the packed read-back of the host path: for every view, or (device candidates) only once a view has to fall back to it
  auto alloc_pack = [&](int n_buffers) -> bool {
    for (int k = 0; k < n_buffers; ++k)
      if (!h_pack[k] && !(h_pack[k] = (uint8_t*)pinned(slot_bytes * B))) return false;
    return true;
  };
  const int n_buffers = n_views > B ? 2 : 1;
  for (int k = 0; k < n_buffers; ++k)
    if (!(h_state[k] = (int32_t*)pinned((size_t)B * kMeshStateWords * 4))) return LMX_ERR_HIP;
  if (!device_candidates && !alloc_pack(n_buffers)) return LMX_ERR_HIP;
  pa.mask0 = d_mask; pa.state = d_state; pa.slot_bytes = slot_bytes; pa.n_levels = L; pa.n_mod = M; pa.n_cg = n_cg; pa.W = W0; pa.H = H0;
  // device candidates: per batch one record buffer in device memory, lists reserved on a bump counter, copied to a pinned buffer by a
  // kernel; sized for every window the kernel takes (<= kMaxWindowPixels records each), so a list that does not fit is not expected
  TrainCandArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  train_cand::ListHeader* h_headers[2] = {nullptr, nullptr};
  train_cand::Record* h_records[2] = {nullptr, nullptr};
  const size_t lists_per_view = (size_t)L * M;
  if (device_candidates) {
    size_t per_view = 0;
    for (int l = 0; l < L; ++l) per_view += (size_t)M * std::min<size_t>((size_t)(W0 >> l) * (H0 >> l), train_cand::kMaxWindowPixels);
    const size_t cap = (per_view * B + 1) & ~(size_t)1;
    TM_ALLOC(d_headers, train_cand::ListHeader*, (size_t)B * lists_per_view * sizeof(train_cand::ListHeader));
    TM_ALLOC(d_records, train_cand::Record*, cap * sizeof(train_cand::Record));
    TM_ALLOC(d_bump, uint32_t*, 4);
    for (int k = 0; k < n_buffers; ++k) {
      h_headers[k] = (train_cand::ListHeader*)pinned((size_t)B * lists_per_view * sizeof(train_cand::ListHeader));
      h_records[k] = (train_cand::Record*)pinned(cap * sizeof(train_cand::Record));
      if (!h_headers[k] || !h_records[k]) return LMX_ERR_HIP;
    }
    std::memcpy(ca.quant, pa.quant, sizeof(ca.quant)); std::memcpy(ca.mag, pa.mag, sizeof(ca.mag));
    ca.mask0 = d_mask; ca.state = d_state; ca.headers = d_headers; ca.records = d_records; ca.bump = d_bump; ca.cap = (uint32_t)cap;
    ca.n_levels = L; ca.n_mod = M; ca.W = W0; ca.H = H0;
    for (int m = 0; m < M; ++m) { ca.strong_threshold[m] = bank->mods[m].strong_threshold; ca.extract_threshold[m] = bank->mods[m].extract_threshold; }
  }

  // renders and quantises `n` views and queues the read-back into buffer k: the candidate lists, or the packed windows
  auto issue = [&](const lmx_mesh_view* vsrc, int n, int k, bool lists) -> lmx_status {
    TR_HIP(hipMemcpyAsync(d_views, vsrc, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice, s));
    launch_mesh_raster(s, d_tri, n_tri, dc, d_views, n, L, d_work, d_state, d_gray, d_depth, d_mask);
    for (int m = 0; m < M; ++m) {
      const lmx_modality_desc& md = bank->mods[m];
      if (md.type == LMX_MOD_COLOR_GRADIENT) {
        const uint8_t* src = d_gray;
        for (int l = 0; l < L; ++l) {
          uint8_t* next = l + 1 < L ? d_pyr[m][l + 1] : nullptr;
          launch_color_quantize(s, src, (uint8_t*)pa.quant[l][m], next, H0 >> l, W0 >> l, n, md.weak_threshold, (float*)pa.mag[l][m], nullptr, nullptr, 1, 0);
          src = next;
        }
      } else {
        launch_depth_quantize(s, d_depth, (uint8_t*)pa.quant[0][m], nullptr, H0, W0, n, md.distance_threshold, md.difference_threshold, d_bins);
      }
    }
    void* dp = nullptr;
    if (lists) {
      TR_HIP(hipMemsetAsync(ca.bump, 0, 4, s));
      launch_train_candidates(s, ca, n);
      TR_HIP(hipHostGetDevicePointer(&dp, h_records[k], 0));
      launch_train_cand_copy(s, ca, (train_cand::Record*)dp);
      TR_HIP(hipMemcpyAsync(h_headers[k], ca.headers, (size_t)n * lists_per_view * sizeof(train_cand::ListHeader), hipMemcpyDeviceToHost, s));
    } else {
      MeshPackArgs a = pa;
      TR_HIP(hipHostGetDevicePointer(&dp, h_pack[k], 0));
      a.out = (uint8_t*)dp;
      launch_mesh_pack(s, a, n);
    }
    TR_HIP(hipGetLastError());
    TR_HIP(hipMemcpyAsync(h_state[k], d_state, (size_t)n * kMeshStateWords * 4, hipMemcpyDeviceToHost, s));
    return LMX_OK;
  };

  // LMX_MESH_TRAIN_TIMING=1: one line on stderr per call (scripts/mesh_train_bench.py reads it): where the call's wall time went
  const bool timing = std::getenv("LMX_MESH_TRAIN_TIMING") != nullptr;
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const clk::time_point t_call = clk::now();
  double wait_ms = 0.0, select_ms = 0.0;
  int n_batches = 0;
  int n_threads = kMeshTrainThreads;
  if (const char* e = std::getenv("LMX_TRAIN_THREADS")) n_threads = std::min(16, std::max(1, std::atoi(e)));
  CopyPool pool(n_threads - 1);
  std::vector<int32_t> templates, features, ids;
  ids.assign((size_t)n_views, -1);
  std::vector<int> accepted_views;
  std::vector<int32_t> acc_rect;
  std::vector<uint16_t> acc_centre;
  const int32_t existing = lmx_bank_num_templates(bank, class_id);
  int32_t next_id = existing, fb = 0;
  // what a pass leaves per view; the templates are collected in view order when every pass is done
  std::vector<ViewResult> all((size_t)n_views);
  std::vector<int32_t> view_box((size_t)n_views * 4);
  std::vector<uint16_t> view_centre((size_t)n_views);
  std::vector<int> fallback;                 // views whose lists carry a status: trained by the pack-and-host path in a second pass
  int64_t n_candidates = 0, list_bytes = 0;
  // One pass over views[idx[0 .. nv)] (idx == null: all views) in batches of B, the read-back of batch b + 1 queued while the host selects
  // on batch b.
  auto run_pass = [&](const int* idx, int nv, bool lists) -> lmx_status {
    std::vector<lmx_mesh_view> picked;
    const lmx_mesh_view* vsrc = views;
    if (idx) {
      picked.resize((size_t)nv);
      for (int i = 0; i < nv; ++i) picked[(size_t)i] = views[idx[i]];
      vsrc = picked.data();
    }
    lmx_status st = issue(vsrc, std::min(B, nv), 0, lists);
    if (st != LMX_OK) return st;
    for (int first = 0, k = 0; first < nv; first += B, k ^= 1) {
      const int n = std::min(B, nv - first);
      const clk::time_point t_wait = clk::now();
      TR_HIP(hipStreamSynchronize(s));   // batch `first` is in buffer k (h_pack or h_records / h_headers, h_state); the device buffers are free again
      wait_ms += ms_since(t_wait); ++n_batches;
      if (first + B < nv) {
        st = issue(vsrc + first + B, std::min(B, nv - first - B), k ^ 1, lists);
        if (st != LMX_OK) return st;
      }
      const int32_t* stw = h_state[k];
      auto view_of = [&](int i) { return idx ? idx[first + i] : first + i; };
      for (int i = 0; i < n; ++i)
        if (stw[(size_t)i * kMeshStateWords + MS_INVALID]) {
          set_error("lmx_bank_train_mesh: view %d puts a vertex at or behind the camera (Z <= 0.01); nothing was added", view_of(i));
          return LMX_ERR_INVALID_ARG;
        }
      const uint8_t* pack = h_pack[k];
      const train_cand::ListHeader* headers = h_headers[k];
      const train_cand::Record* records = h_records[k];
      std::vector<uint8_t> needs_pack((size_t)n, 0);
      const clk::time_point t_sel = clk::now();
      pool.parallel_for(n, [&](int i) {
        ViewResult& r = all[(size_t)view_of(i)];
        try {
          if (lists) needs_pack[(size_t)i] = !select_view_from_lists(bank, headers + (size_t)i * lists_per_view, records, ca.cap, stw + (size_t)i * kMeshStateWords, W0, H0, r);
          else select_view(bank, pack + (size_t)i * slot_bytes, stw + (size_t)i * kMeshStateWords, W0, H0, r);
        } catch (const std::exception& e) {
          r.status = LMX_ERR_INVALID_ARG; r.error = e.what();
        }
      });
      select_ms += ms_since(t_sel);
      for (int i = 0; i < n; ++i) {
        const int v = view_of(i);
        const ViewResult& r = all[(size_t)v];
        if (r.status != LMX_OK) { set_error("lmx_bank_train_mesh: view %d: %s", v, r.error.c_str()); return r.status; }
        std::memcpy(&view_box[(size_t)v * 4], stw + (size_t)i * kMeshStateWords + MS_LEVEL, 16);
        view_centre[(size_t)v] = (uint16_t)stw[(size_t)i * kMeshStateWords + MS_CENTRE_DEPTH];
        if (needs_pack[(size_t)i]) { fallback.push_back(v); continue; }
        if (lists) {
          list_bytes += (int64_t)(lists_per_view * sizeof(train_cand::ListHeader));
          for (size_t j = 0; j < lists_per_view; ++j) {
            const uint32_t nc = headers[(size_t)i * lists_per_view + j].n_cands;
            n_candidates += nc; list_bytes += (int64_t)nc * (int64_t)sizeof(train_cand::Record);
          }
        }
      }
    }
    return LMX_OK;
  };
  lmx_status st = run_pass(nullptr, n_views, device_candidates);
  if (st != LMX_OK) return st;
  const int n_fallback = (int)fallback.size();
  if (n_fallback) {   // the rasteriser is deterministic: these views are simply rendered again, for the packed read-back
    if (!alloc_pack(std::min(n_buffers, n_fallback > B ? 2 : 1))) return LMX_ERR_HIP;
    const std::vector<int> again(fallback);
    st = run_pass(again.data(), n_fallback, false);
    if (st != LMX_OK) return st;
  }
  for (int v = 0; v < n_views; ++v) {
    ViewResult& r = all[(size_t)v];
    if (!r.accepted) continue;
    for (size_t t = 0; t < r.templates.size(); t += 5) r.templates[t + 3] += fb;
    templates.insert(templates.end(), r.templates.begin(), r.templates.end());
    features.insert(features.end(), r.features.begin(), r.features.end());
    fb += (int32_t)(r.features.size() / 3);
    ids[(size_t)v] = next_id++;
    accepted_views.push_back(v);
    const int32_t* b = &view_box[(size_t)v * 4];
    acc_rect.insert(acc_rect.end(), {b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1});   // an accepted view has covered pixels
    acc_centre.push_back(view_centre[(size_t)v]);
    std::vector<int32_t>().swap(r.templates); std::vector<int32_t>().swap(r.features);
  }
  const size_t n_acc = accepted_views.size();
  if (side_car) {
    lmx_renderer_params* p = side.get();
    p->n_templates = n_acc;
    p->obj_origin_dists = new double[n_acc](); p->rects = new int32_t[n_acc * 4](); p->distances = new double[n_acc]();
    p->R = new double[n_acc * 9](); p->T = new double[n_acc * 3](); p->K = new double[n_acc * 9]();
    for (size_t i = 0; i < n_acc; ++i) {
      const lmx_mesh_view& v = views[accepted_views[i]];
      p->obj_origin_dists[i] = v.distance;
      std::memcpy(p->rects + i * 4, &acc_rect[i * 4], 16);
      p->distances[i] = v.distance - double((float)acc_centre[i] / 1000.0f);   // src/renderer.cpp:284
      std::memcpy(p->R + i * 9, v.R, sizeof(v.R));
      p->T[i * 3 + 0] = 0.0; p->T[i * 3 + 1] = 0.0; p->T[i * 3 + 2] = v.distance;
      const double K[9] = {(double)(float)cam->fx, 0.0, (double)((float)W0 / 2.0f), 0.0, (double)(float)cam->fy, (double)((float)H0 / 2.0f), 0.0, 0.0, 1.0};
      std::memcpy(p->K + i * 9, K, sizeof(K));
    }
  }
  if (n_acc) {
    st = lmx_bank_add_class(bank, class_id, (int32_t)n_acc, templates.data(), features.data(), fb);
    if (st != LMX_OK) return st;
  }
  if (template_ids) std::memcpy(template_ids, ids.data(), ids.size() * sizeof(int32_t));
  if (side_car) *side_car = side.release();
  const double total_ms = ms_since(t_call);
  if (stats) {
    stats->n_accepted = (int32_t)n_acc;
    stats->n_device_views = device_candidates ? n_views - n_fallback : 0;
    stats->n_fallback_views = n_fallback;
    stats->n_candidates = n_candidates; stats->list_bytes = list_bytes;
    stats->total_ms = total_ms; stats->device_wait_ms = wait_ms; stats->host_select_ms = select_ms;
  }
  if (timing)
    std::fprintf(stderr, "lmx_bank_train_mesh timing: views %d accepted %zu batches %d of %d total_ms %.3f device_wait_ms %.3f host_select_ms %.3f (%d threads) "
                 "device_bytes %zu pinned_bytes %zu candidates %s device_views %d fallback_views %d n_candidates %lld list_bytes %lld\n", n_views, n_acc, n_batches, B,
                 total_ms, wait_ms, select_ms, pool.threads(), device_bytes, pinned_bytes, device_candidates ? "device" : "host",
                 device_candidates ? n_views - n_fallback : 0, n_fallback, (long long)n_candidates, (long long)list_bytes);
  return LMX_OK;
}
#undef TM_ALLOC

}  // namespace lmx

extern "C" lmx_status lmx_bank_add_template(lmx_bank* bank, int32_t device, const lmx_image* sources, int32_t n_sources, const char* class_id,
                                            const lmx_image* object_mask, int32_t* template_id, int32_t bounding_box[4]) {
  return lmx::guarded("lmx_bank_add_template", [&]() -> lmx_status {
  if (!bank || !sources || !class_id || !template_id) { lmx::set_error("lmx_bank_add_template: null argument"); return LMX_ERR_INVALID_ARG; }
  return lmx::train_add_template(bank, device, sources, n_sources, class_id, object_mask, template_id, bounding_box);
  });
}

extern "C" lmx_status lmx_bank_train_mesh(lmx_bank* bank, int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam,
                                          const lmx_mesh_view* views, int32_t n_views, const char* class_id, int32_t* template_ids,
                                          lmx_renderer_params** side_car) {
  return lmx::guarded("lmx_bank_train_mesh", [&]() -> lmx_status {
  if (!bank || !class_id) { lmx::set_error("lmx_bank_train_mesh: null argument"); return LMX_ERR_INVALID_ARG; }
  lmx::mr::Camera dc;
  const lmx_status st = lmx::mesh_check_args("lmx_bank_train_mesh", triangles, n_triangles, cam, views, n_views, &dc);
  if (st != LMX_OK) return st;
  return lmx::train_mesh(bank, device, triangles, n_triangles, cam, dc, views, n_views, class_id, template_ids, side_car, false, nullptr);
  });
}

extern "C" lmx_status lmx_bank_train_mesh_opts(lmx_bank* bank, int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam,
                                               const lmx_mesh_view* views, int32_t n_views, const char* class_id, int32_t* template_ids,
                                               lmx_renderer_params** side_car, const lmx_train_mesh_opts* opts, lmx_train_mesh_stats* stats) {
  return lmx::guarded("lmx_bank_train_mesh_opts", [&]() -> lmx_status {
  if (!bank || !class_id) { lmx::set_error("lmx_bank_train_mesh: null argument"); return LMX_ERR_INVALID_ARG; }
  if (opts && (opts->struct_size < sizeof(lmx_train_mesh_opts) || (opts->candidates != LMX_TRAIN_CANDIDATES_HOST && opts->candidates != LMX_TRAIN_CANDIDATES_DEVICE))) {
    lmx::set_error("lmx_bank_train_mesh_opts: struct_size %u, candidates %d are not valid options", opts->struct_size, opts->candidates);
    return LMX_ERR_INVALID_ARG;
  }
  lmx::mr::Camera dc;
  const lmx_status st = lmx::mesh_check_args("lmx_bank_train_mesh", triangles, n_triangles, cam, views, n_views, &dc);
  if (st != LMX_OK) return st;
  return lmx::train_mesh(bank, device, triangles, n_triangles, cam, dc, views, n_views, class_id, template_ids, side_car,
                         opts && opts->candidates == LMX_TRAIN_CANDIDATES_DEVICE, stats);
  });
}

// The production kernel and the production rank-and-select on one caller-supplied window (the whole image): tests/test_gpu_train_candidates.py
extern "C" lmx_status lmx_debug_train_extract(int32_t device, const uint8_t* label, const float* mag, const uint8_t* mask, int32_t H, int32_t W, int32_t num_features,
                                              float strong_threshold, int32_t extract_threshold, uint32_t* records, size_t cap, size_t* n_records,
                                              uint32_t* label_counts, uint32_t* area, int32_t* features, int32_t* n_features, int32_t* accepted) {
  return lmx::guarded("lmx_debug_train_extract", [&]() -> lmx_status {
    using namespace lmx;
    namespace tc = train_cand;
    if (!label || !records || !n_records || !label_counts || !area || !features || !n_features || !accepted) { set_error("lmx_debug_train_extract: null argument"); return LMX_ERR_INVALID_ARG; }
    if (H < 1 || W < 1 || !tc::window_fits(W, H)) { set_error("lmx_debug_train_extract: a %d x %d window is outside the device path (rows padded to 4 pixels, at most %d bytes)", W, H, 4 * tc::kMaxWindowDwords); return LMX_ERR_SHAPE; }
    { std::string why; if (!train_select::check_num_features({train_select::Modality{mag != nullptr, num_features, strong_threshold, extract_threshold}}, 1, &why)) { set_error("lmx_debug_train_extract: %s", why.c_str()); return LMX_ERR_SHAPE; } }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
    TR_HIP(hipSetDevice(device));
    const size_t px = (size_t)H * W, cap_dev = std::min<size_t>((cap + 1) & ~(size_t)1, (size_t)tc::kMaxWindowPixels);
    std::vector<void*> to_free;
    struct Free { std::vector<void*>& v; ~Free() { for (void* p : v) (void)hipFree(p); } } free_all{to_free};
    auto dmalloc = [&](size_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, std::max<size_t>(bytes, 256) + 64) != hipSuccess) return nullptr; to_free.push_back(p); return p; };
    uint8_t* d_label = (uint8_t*)dmalloc(px);
    float* d_mag = mag ? (float*)dmalloc(px * 4) : nullptr;
    uint8_t* d_mask = mask ? (uint8_t*)dmalloc(px) : nullptr;
    int32_t* d_state = (int32_t*)dmalloc(kMeshStateWords * 4);
    tc::ListHeader* d_header = (tc::ListHeader*)dmalloc(sizeof(tc::ListHeader));
    tc::Record* d_records = (tc::Record*)dmalloc((cap_dev + 2) * sizeof(tc::Record));
    uint32_t* d_bump = (uint32_t*)dmalloc(4);
    if (!d_label || (mag && !d_mag) || (mask && !d_mask) || !d_state || !d_header || !d_records || !d_bump) { set_error("hipMalloc failed"); return LMX_ERR_HIP; }
    int32_t state[kMeshStateWords] = {};
    state[MS_LEVEL + 0] = 0; state[MS_LEVEL + 1] = 0; state[MS_LEVEL + 2] = W - 1; state[MS_LEVEL + 3] = H - 1;   // mesh_window: the whole image
    TR_HIP(hipMemcpy(d_label, label, px, hipMemcpyHostToDevice));
    if (mag) TR_HIP(hipMemcpy(d_mag, mag, px * 4, hipMemcpyHostToDevice));
    if (mask) TR_HIP(hipMemcpy(d_mask, mask, px, hipMemcpyHostToDevice));
    TR_HIP(hipMemcpy(d_state, state, sizeof(state), hipMemcpyHostToDevice));
    TR_HIP(hipMemset(d_bump, 0, 4));
    TR_HIP(hipMemset(d_header, 0xff, sizeof(tc::ListHeader)));
    TrainCandArgs a;
    std::memset(&a, 0, sizeof(a));
    a.quant[0][0] = d_label; a.mag[0][0] = d_mag; a.mask0 = d_mask; a.state = d_state; a.headers = d_header; a.records = d_records; a.bump = d_bump;
    a.cap = (uint32_t)cap_dev; a.strong_threshold[0] = strong_threshold; a.extract_threshold[0] = extract_threshold; a.n_levels = 1; a.n_mod = 1; a.W = W; a.H = H;
    launch_train_candidates(nullptr, a, 1);
    TR_HIP(hipGetLastError());
    TR_HIP(hipDeviceSynchronize());
    tc::ListHeader hd;
    TR_HIP(hipMemcpy(&hd, d_header, sizeof(hd), hipMemcpyDeviceToHost));
    if (hd.status == tc::ST_OVERFLOW || (hd.status == 0 && hd.n_cands > cap)) { set_error("lmx_debug_train_extract: %u candidates exceed the capacity %zu", hd.n_cands, cap); return LMX_ERR_OVERFLOW; }
    if (hd.status != 0 || (uint64_t)hd.offset + hd.n_cands > cap_dev) { set_error("lmx_debug_train_extract: list status %u, offset %u", hd.status, hd.offset); return LMX_ERR_HIP; }
    std::vector<tc::Record> recs(hd.n_cands);
    if (hd.n_cands) TR_HIP(hipMemcpy(recs.data(), d_records + hd.offset, recs.size() * sizeof(tc::Record), hipMemcpyDeviceToHost));
    if (hd.n_cands) std::memcpy(records, recs.data(), recs.size() * sizeof(tc::Record));
    *n_records = hd.n_cands;
    std::memcpy(label_counts, hd.label_counts, sizeof(hd.label_counts));
    *area = hd.area;
    std::vector<train_select::Feat> out;
    *accepted = train_select::select_from_list(mag != nullptr, hd, recs.data(), 0, 0, (size_t)num_features, out) ? 1 : 0;
    *n_features = *accepted ? (int32_t)out.size() : 0;
    for (size_t i = 0; *accepted && i < out.size(); ++i) { features[3 * i] = out[i].x; features[3 * i + 1] = out[i].y; features[3 * i + 2] = out[i].label; }
    return LMX_OK;
  });
}
