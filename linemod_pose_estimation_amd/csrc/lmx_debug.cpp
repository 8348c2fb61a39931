// liblmx.so, introspection: stage-level debug reads for the parity tests, counters, per-kernel HIP-event timing, the algorithmic-bytes
// figure of SURVEY.md 8(d), and the test hooks of the std::sort restatement (csrc/lmx_sort_emul.hpp, lmx_sort_block.hpp).

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "lmx_ctx.hpp"
#include "lmx_sort_emul.hpp"

using namespace lmx;

static const char* kKernelNames[K_COUNT] = {"k_pre",            "k_color_quantize", "k_depth_quantize", "k_nn_down2",   "k_spread_linearize",
                                            "k_pack_nibbles",   "k_score_coarse",   "k_refine"};

extern "C" {

lmx_status lmx_ctx_debug_read(lmx_ctx* c, int32_t frame, int32_t what, int32_t level, int32_t modality, void* out, size_t out_bytes) {
  if (!c || !out) { set_error("lmx_ctx_debug_read: null argument"); return LMX_ERR_INVALID_ARG; }
  if (frame < 0 || frame >= c->F || level < 0 || level >= c->L || modality < 0 || modality >= c->M) { set_error("debug_read: index out of range"); return LMX_ERR_INVALID_ARG; }
  LMX_HIP(hipSetDevice(c->device));
  if (sync_lanes(c) != LMX_OK) return LMX_ERR_HIP;
  const LevelGeom& g = c->kp.geom[level];
  if (what == LMX_DBG_QUANTIZED) {
    const size_t n = (size_t)g.W * g.H;
    if (out_bytes < n) { set_error("debug_read: buffer too small"); return LMX_ERR_INVALID_ARG; }
    LMX_HIP(hipMemcpy(out, c->kp.fb.quant[level][modality] + (size_t)frame * n, n, hipMemcpyDeviceToHost));
  } else if (what == LMX_DBG_LINEAR_MEMORY) {
    const size_t n = (size_t)g.T * g.T * g.cells;
    if (out_bytes < 8 * n) { set_error("debug_read: buffer too small"); return LMX_ERR_INVALID_ARG; }
    if (level == c->L - 1) {
      // the coarsest level lives nibble-packed on the device; unpack to upstream's byte-wide linear memories
      const size_t nb = (n + 1) / 2;
      std::vector<uint8_t> nib(nb);
      for (int o = 0; o < 8; ++o) {
        LMX_HIP(hipMemcpy(nib.data(), c->kp.fb.lmn[modality] + (size_t)frame * g.nib_mod_stride + (size_t)o * g.nib_ori_stride, nb,
                          hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) ((uint8_t*)out)[o * n + i] = (uint8_t)((nib[i >> 1] >> (4 * (i & 1))) & 0xf);
      }
    } else {
      // finer levels hold the linearised spread image only; expand it to upstream's eight linear memories for the caller
      static const uint32_t masks[8] = {0x0103070fu, 0x02070f1fu, 0x040e1f3fu, 0x081c3e7fu, 0x10387cfeu, 0x2070f8fdu, 0x40e0f1fbu, 0x80c1e3f7u};
      std::vector<uint8_t> sp(n);
      if (g.ls_bands) {   // banded image: take the first 16 columns of every band row
        std::vector<uint8_t> banded(g.ls_stride);
        LMX_HIP(hipMemcpy(banded.data(), c->kp.fb.ls[level][modality] + (size_t)frame * g.ls_stride, g.ls_stride, hipMemcpyDeviceToHost));
        const size_t rows = n / g.Wc;
        for (size_t r = 0; r < rows; ++r)
          for (uint32_t k = 0; k < g.ls_bands; ++k)
            memcpy(&sp[r * g.Wc + 16 * k], &banded[(size_t)k * g.ls_band_stride + (r + 1) * 32], 16);
      } else
        LMX_HIP(hipMemcpy(sp.data(), c->kp.fb.ls[level][modality] + (size_t)frame * g.ls_stride, n, hipMemcpyDeviceToHost));
      for (int o = 0; o < 8; ++o)
        for (size_t i = 0; i < n; ++i) {
          int r = 0;
          for (int k = 0; k < 4; ++k) r += (sp[i] & ((masks[o] >> (8 * k)) & 0xffu)) != 0;
          ((uint8_t*)out)[o * n + i] = (uint8_t)r;
        }
    }
  } else if (what == LMX_DBG_PYRAMID_BGR) {
    if (c->bank->mods[modality].type != LMX_MOD_COLOR_GRADIENT) { set_error("debug_read: modality %d has no colour pyramid", modality); return LMX_ERR_INVALID_ARG; }
    const size_t n = (size_t)g.W * g.H * c->color_ch;   // [H_l][W_l][3], or [H_l][W_l] for a gray context
    if (out_bytes < n) { set_error("debug_read: buffer too small"); return LMX_ERR_INVALID_ARG; }
    LMX_HIP(hipMemcpy(out, c->mb[modality].bgr[level] + (size_t)frame * n, n, hipMemcpyDeviceToHost));
  } else if (what == LMX_DBG_DEPTH) {
    if (c->bank->mods[modality].type != LMX_MOD_DEPTH_NORMAL) { set_error("debug_read: modality %d has no depth source", modality); return LMX_ERR_INVALID_ARG; }
    const size_t n = (size_t)c->desc.width * c->desc.height * 2;
    if (out_bytes < n) { set_error("debug_read: buffer too small"); return LMX_ERR_INVALID_ARG; }
    LMX_HIP(hipMemcpy(out, (const uint8_t*)c->mb[modality].depth + (size_t)frame * n, n, hipMemcpyDeviceToHost));
  } else if (what == LMX_DBG_RAW_SPREAD || what == LMX_DBG_RAW_NIBBLES || what == LMX_DBG_RAW_BYTES) {
    // a whole allocation of lmx_ctx.cpp's frame buffers, untouched: the sizes are the ones dev_alloc got there
    if (frame != 0) { set_error("debug_read: a raw read returns every frame, frame must be 0"); return LMX_ERR_INVALID_ARG; }
    const LevelGeom& gc = c->kp.geom[c->L - 1];
    const uint8_t* src = nullptr;
    size_t n = 0;
    if (what == LMX_DBG_RAW_SPREAD) {
      if (level >= c->L - 1) { set_error("debug_read: the coarsest level %d keeps no spread image", level); return LMX_ERR_INVALID_ARG; }
      src = c->kp.fb.ls[level][modality];
      n = (size_t)c->F * g.ls_stride + 8192;
    } else if (what == LMX_DBG_RAW_NIBBLES) {
      src = c->kp.fb.lmn[0];
      n = (size_t)c->M * c->F * gc.nib_mod_stride + 8192;
    } else {
      if (spread_writes_nibbles(gc)) { set_error("debug_read: this context keeps no byte-wide memories, its spread kernel writes the nibbles itself"); return LMX_ERR_INVALID_ARG; }
      src = c->kp.fb.lm[c->L - 1][modality];
      n = (size_t)c->F * gc.mod_stride + 8192;
    }
    if (!src) { set_error("debug_read: the context holds no such buffer"); return LMX_ERR_INVALID_ARG; }
    if (out_bytes < n) { set_error("debug_read: buffer too small, the allocation has %zu bytes", n); return LMX_ERR_INVALID_ARG; }
    LMX_HIP(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
  } else {
    set_error("debug_read: unknown item %d", what);
    return LMX_ERR_INVALID_ARG;
  }
  return LMX_OK;
}

lmx_status lmx_ctx_debug_enqueue_labels(lmx_ctx* c, int32_t n_frames, const uint8_t* const* labels, int32_t n_labels, float threshold, const float* thresholds,
                                        int32_t n_thresholds, const char* const* class_ids, int32_t n_class_ids) {
  return lmx::guarded("lmx_ctx_debug_enqueue_labels", [&]() -> lmx_status {
  if (!c) { set_error("lmx_ctx_debug_enqueue_labels: null context"); return LMX_ERR_INVALID_ARG; }
  if (n_frames < 1 || n_frames > c->F) { set_error("lmx_ctx_debug_enqueue_labels: n_frames=%d outside [1,%d]", n_frames, c->F); return LMX_ERR_INVALID_ARG; }
  if (!labels || n_labels != c->L * c->M) {
    set_error("lmx_ctx_debug_enqueue_labels: %d label arrays for %d levels x %d modalities (labels[level * n_modalities + modality])", labels ? n_labels : 0, c->L, c->M);
    return LMX_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_labels; ++i)
    if (!labels[i]) { set_error("lmx_ctx_debug_enqueue_labels: label array %d (level %d, modality %d) is null", i, i / c->M, i % c->M); return LMX_ERR_INVALID_ARG; }
  return ctx_enqueue_labels(c, n_frames, labels, threshold, thresholds, n_thresholds, class_ids, n_class_ids);
  });
}

lmx_status lmx_debug_launch_helper_counters(lmx_ctx* c, uint64_t out[3]) {
  if (!c || !out) { set_error("lmx_debug_launch_helper_counters: null argument"); return LMX_ERR_INVALID_ARG; }
  out[0] = out[1] = out[2] = 0;   // no one-frame call yet: the context has no helper
  if (c->launch_helper) {
    const LaunchHelper::Counters k = c->launch_helper->counters();
    out[0] = k.jobs; out[1] = k.sleeps; out[2] = k.notifies;
  }
  return LMX_OK;
}

lmx_status lmx_debug_orientation_labels(int32_t device, const int16_t* dx, const int16_t* dy, size_t n, uint8_t* out) {
  if (!dx || !dy || !out) { set_error("lmx_debug_orientation_labels: null argument"); return LMX_ERR_INVALID_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  LMX_HIP(hipSetDevice(device));
  short *d_dx = nullptr, *d_dy = nullptr;
  uint8_t* d_out = nullptr;
  lmx_status st = LMX_OK;
  auto run = [&]() -> lmx_status {
    LMX_HIP(hipMalloc((void**)&d_dx, n * 2));
    LMX_HIP(hipMalloc((void**)&d_dy, n * 2));
    LMX_HIP(hipMalloc((void**)&d_out, n));
    LMX_HIP(hipMemcpy(d_dx, dx, n * 2, hipMemcpyHostToDevice));
    LMX_HIP(hipMemcpy(d_dy, dy, n * 2, hipMemcpyHostToDevice));
    launch_debug_orientation_label(nullptr, d_dx, d_dy, d_out, n);
    LMX_HIP(hipDeviceSynchronize());
    LMX_HIP(hipMemcpy(out, d_out, n, hipMemcpyDeviceToHost));
    return LMX_OK;
  };
  st = run();
  (void)hipFree(d_dx); (void)hipFree(d_dy); (void)hipFree(d_out);
  return st;
}

lmx_status lmx_debug_depth_normal_bins(int32_t device, const uint16_t* taps, size_t n, int32_t distance_threshold, int32_t difference_threshold,
                                       int32_t variant, const uint8_t* normal_lut, uint8_t* out_bins) {
  if (n > 0 && (!taps || !out_bins)) { set_error("lmx_debug_depth_normal_bins: null argument"); return LMX_ERR_INVALID_ARG; }
  if (variant != LMX_DBG_DEPTH_INT && variant != LMX_DBG_DEPTH_INT64 && variant != LMX_DBG_DEPTH_PIPELINED) {
    set_error("lmx_debug_depth_normal_bins: unknown variant %d", variant);
    return LMX_ERR_INVALID_ARG;
  }
  if (variant != LMX_DBG_DEPTH_INT64 && difference_threshold > 200) {
    set_error("lmx_debug_depth_normal_bins: the int32 forms hold for difference_threshold <= 200 only (got %d)", difference_threshold);
    return LMX_ERR_INVALID_ARG;
  }
  if (n > ((size_t)1 << 28)) { set_error("lmx_debug_depth_normal_bins: at most 2^28 tuples per call"); return LMX_ERR_INVALID_ARG; }
  std::vector<uint8_t> lut(LMX_NORMAL_LUT_SIZE), bins;
  if (normal_lut) std::memcpy(lut.data(), normal_lut, LMX_NORMAL_LUT_SIZE);
  else default_normal_lut(lut.data());
  if (!normal_bins_device_image(lut.data(), bins)) { set_error("lmx_debug_depth_normal_bins: a table entry is neither 0 nor one bit"); return LMX_ERR_INVALID_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  if (n == 0) return LMX_OK;
  LMX_HIP(hipSetDevice(device));
  // tuple c's nine values go to elements 45 (c / 5) + c % 5 + 5 k, k = 0..8 (launch_debug_depth_normal_bins)
  const size_t groups = (n + kDebugDepthPatchGroup - 1) / kDebugDepthPatchGroup;
  std::vector<uint16_t> patches(groups * kDebugDepthPatchElems, 0);
  for (size_t c = 0; c < n; ++c) {
    uint16_t* p = &patches[(c / kDebugDepthPatchGroup) * kDebugDepthPatchElems + c % kDebugDepthPatchGroup];
    const uint16_t* t = taps + 9 * c;   // d, then the eight neighbours in DepthTaps order: the pixel sits in the middle of them
    for (int k = 0; k < 4; ++k) p[5 * k] = t[1 + k];
    p[20] = t[0];
    for (int k = 4; k < 8; ++k) p[5 * (k + 1)] = t[1 + k];
  }
  uint16_t* d_patches = nullptr;
  uint8_t *d_bins = nullptr, *d_out = nullptr;
  auto run = [&]() -> lmx_status {
    LMX_HIP(hipMalloc((void**)&d_patches, patches.size() * 2));
    LMX_HIP(hipMalloc((void**)&d_bins, bins.size()));
    LMX_HIP(hipMalloc((void**)&d_out, n));
    LMX_HIP(hipMemcpy(d_patches, patches.data(), patches.size() * 2, hipMemcpyHostToDevice));
    LMX_HIP(hipMemcpy(d_bins, bins.data(), bins.size(), hipMemcpyHostToDevice));
    launch_debug_depth_normal_bins(nullptr, d_patches, n, distance_threshold, difference_threshold, variant, d_bins, d_out);
    LMX_HIP(hipGetLastError());
    LMX_HIP(hipDeviceSynchronize());
    LMX_HIP(hipMemcpy(out_bins, d_out, n, hipMemcpyDeviceToHost));
    return LMX_OK;
  };
  const lmx_status st = run();
  (void)hipFree(d_patches); (void)hipFree(d_bins); (void)hipFree(d_out);
  return st;
}

lmx_status lmx_debug_bank_tables(const lmx_bank* bank, int32_t width, int32_t height, int32_t max_batch, int32_t shard_rank, int32_t shard_world, int32_t ls_flat,
                                 int32_t table, void* out, size_t out_bytes, size_t* n_bytes, uint64_t* fnv1a) {
  return lmx::guarded("lmx_debug_bank_tables", [&]() -> lmx_status {
  if (!bank || bank->T.empty() || bank->T.size() > (size_t)kMaxLevels || bank->mods.empty() || bank->mods.size() > (size_t)kMaxModalities || max_batch < 1 ||
      shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world) {
    set_error("lmx_debug_bank_tables: invalid argument");
    return LMX_ERR_INVALID_ARG;
  }
  const int L = (int)bank->T.size();
  LevelGeom geom[kMaxLevels] = {};
  if (lmx_status st = build_geometry(*bank, width, height, ls_flat != 0, geom)) return st;
  BankTables t;
  build_bank_tables(*bank, geom, max_batch, shard_rank, shard_world, &t);
  static_assert(sizeof(LevelGeom) == 64, "LMX_TAB_SUMMARY documents 16 words per level");
  std::vector<uint32_t> summary = {(uint32_t)t.G, (uint32_t)t.nf_max_coarse, (uint32_t)t.uni_ok, t.uni_mod_block_bytes, (uint32_t)L, (uint32_t)bank->mods.size(), (uint32_t)t.class_names.size(), 0u};
  summary.resize(8 + 16 * (size_t)L);
  std::memcpy(summary.data() + 8, geom, (size_t)L * sizeof(LevelGeom));
  auto bytes = [](const auto& v) { return std::pair<const void*, size_t>(v.data(), v.size() * sizeof(v[0])); };
  const std::pair<const void*, size_t> tables[] = {bytes(t.info),  bytes(t.linfo), bytes(t.coarse_off),  bytes(t.coarse_uni), bytes(t.coarse_blk),
                                                   bytes(t.sinfo), bytes(t.feat),  bytes(t.feat_count), bytes(summary)};   // LMX_TAB_* order
  if (table < 0 || table > LMX_TAB_SUMMARY) { set_error("lmx_debug_bank_tables: unknown table %d", table); return LMX_ERR_INVALID_ARG; }
  const void* p = tables[table].first;
  const size_t n = tables[table].second;
  if (n_bytes) *n_bytes = n;
  if (fnv1a) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const uint8_t*>(p)[i]) * 0x100000001b3ull;
    *fnv1a = h;
  }
  if (out) {
    if (out_bytes < n) { set_error("lmx_debug_bank_tables: the table has %zu bytes, the buffer %zu", n, out_bytes); return LMX_ERR_INVALID_ARG; }
    if (n) std::memcpy(out, p, n);
  }
  return LMX_OK;
  });
}

lmx_status lmx_ctx_stats(lmx_ctx* c, int64_t* n_candidates, int64_t* n_raw_matches) {
  if (!c) { set_error("lmx_ctx_stats: null context"); return LMX_ERR_INVALID_ARG; }
  if (n_candidates) *n_candidates = c->stat_cands;
  if (n_raw_matches) *n_raw_matches = c->stat_matches;
  return LMX_OK;
}

int32_t lmx_num_kernels(void) { return K_COUNT; }
const char* lmx_kernel_name(int32_t id) { return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : nullptr; }
const char* lmx_ctx_device_kernel_name(lmx_ctx* c, int32_t id) {
  if (!c || id < 0 || id >= K_COUNT) return nullptr;
  if (id == K_SCORE_COARSE) {
    const int v = score_kernel_variant(c->dbank);
    return v == 2 ? "k_score_coarse_sb" : (v == 1 ? "k_score_coarse_u8" : "k_score_coarse");
  }
  if (id == K_SPREAD_LINEARIZE) return "k_spread_linearize_t";
  return kKernelNames[id];
}
lmx_status lmx_ctx_set_profiling(lmx_ctx* c, int32_t enabled) {
  if (!c) { set_error("null context"); return LMX_ERR_INVALID_ARG; }
  c->profiling = (uint32_t)enabled;
  return LMX_OK;
}
lmx_status lmx_ctx_kernel_time(lmx_ctx* c, int32_t id, double* total_ms, int64_t* launches) {
  if (!c || id < 0 || id >= K_COUNT) { set_error("lmx_ctx_kernel_time: bad argument"); return LMX_ERR_INVALID_ARG; }
  if (total_ms) *total_ms = c->k_ms[id];
  if (launches) *launches = c->k_launches[id];
  return LMX_OK;
}
lmx_status lmx_ctx_reset_profiling(lmx_ctx* c) {
  if (!c) { set_error("null context"); return LMX_ERR_INVALID_ARG; }
  for (int i = 0; i < K_COUNT; ++i) { c->k_ms[i] = 0; c->k_launches[i] = 0; }
  return LMX_OK;
}

// Algorithmic bytes per enqueue for one kernel: what the stage must read and write if every
// byte moved exactly once.  For k_score_coarse: sum over templates and modalities of nf * template_positions
// (one linear-memory byte per feature per placement) + the u8 map per modality and the u16 total per placement.
lmx_status lmx_ctx_algorithmic_bytes(lmx_ctx* c, int32_t id, int32_t n_frames, double* bytes) {
  if (!c || !bytes || id < 0 || id >= K_COUNT) { set_error("lmx_ctx_algorithmic_bytes: bad argument"); return LMX_ERR_INVALID_ARG; }
  const lmx_bank* b = c->bank;
  const int L = c->L, M = c->M, per = L * M;
  double v = 0;
  const LevelGeom& g0 = c->kp.geom[0];
  int n_cg = 0, n_dn = 0;
  for (int m = 0; m < M; ++m) (b->mods[m].type == LMX_MOD_COLOR_GRADIENT ? n_cg : n_dn)++;
  switch (id) {
    case K_PRE: v = 0; break;  // depends on the raw frame size passed to upload_raw
    case K_COLOR_QUANTIZE:  // 3 B in + 1 B out per pixel, + 3/4 B for the pyrDown output of the next level (gray: 1 B in, 1/4 B pyrDown)
      for (int l = 0; l < L; ++l)
        v += n_cg * (c->color_ch + 1.0 + (l + 1 < L ? c->color_ch * 0.25 : 0.0)) * c->kp.geom[l].W * c->kp.geom[l].H;
      break;
    case K_DEPTH_QUANTIZE: v = n_dn * 3.0 * g0.W * g0.H; break;
    case K_NN_DOWN:
      for (int l = 1; l < L; ++l) v += n_dn * 2.0 * c->kp.geom[l].W * c->kp.geom[l].H;
      break;
    case K_SPREAD_LINEARIZE:  // 1 B in; at the coarsest level eight response maps out (4 B/px nibble-packed, 8 B/px in the generic
                              // byte path), 1 B out (spread byte) at finer levels
      for (int l = 0; l < L; ++l)
        v += M * (l == L - 1 ? (spread_writes_nibbles(c->kp.geom[l]) ? 5.0 : 9.0) : 2.0) * c->kp.geom[l].W * c->kp.geom[l].H;
      break;
    case K_PACK_NIBBLES: v = spread_writes_nibbles(c->kp.geom[L - 1]) ? 0.0 : M * 12.0 * c->kp.geom[L - 1].W * c->kp.geom[L - 1].H; break;  // generic path only
    case K_SCORE_COARSE: {
      const LevelGeom& g = c->kp.geom[L - 1];
      for (const auto& kv : b->classes) {
        const ClassData& cd = kv.second;
        long begin, end;
        shard_range(cd.n_pyramids, c->desc.shard_rank, c->desc.shard_world, &begin, &end);
        for (long t = begin; t < end; ++t)
          for (int m = 0; m < M; ++m) {
            const TemplateRow tm = template_row(cd, per, t, (L - 1) * M + m);
            v += tm.feat_count * (double)template_positions(g, tm.width, tm.height) + 3.0 * g.cells;
          }
      }
      break;
    }
    case K_REFINE: v = 0; break;  // depends on the candidate count of the frame; reported from stats by the caller
  }
  *bytes = v * n_frames;
  return LMX_OK;
}

}  // extern "C"

// Test hooks for csrc/lmx_sort_emul.hpp (host build of the code the device runs): the permutation the restated introsort
// produces for Match::operator< on (similarity, template_id) and for the cluster comparator score-descending.
extern "C" {
lmx_status lmx_debug_introsort_perm(const float* similarity, const int32_t* template_id, int32_t n, int32_t* perm) {
  if (n < 0 || (n > 0 && (!similarity || !template_id || !perm))) { set_error("lmx_debug_introsort_perm: invalid argument"); return LMX_ERR_INVALID_ARG; }
  for (int32_t i = 0; i < n; ++i) perm[i] = i;
  lmx::sortemu::sort(perm, n, [&](int32_t a, int32_t b) { return similarity[a] != similarity[b] ? similarity[a] > similarity[b] : template_id[a] < template_id[b]; });
  return LMX_OK;
}
lmx_status lmx_debug_device_sort_perm(int32_t device, const float* similarity, const int32_t* template_id, int32_t n, int32_t* perm) {
  if (n < 0 || n > F2_MAX || (n > 0 && (!similarity || !template_id || !perm))) { set_error("lmx_debug_device_sort_perm: invalid argument (n <= %d)", F2_MAX); return LMX_ERR_INVALID_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  if (n == 0) return LMX_OK;
  LMX_HIP(hipSetDevice(device));
  float* d_sim = nullptr; int* d_tid = nullptr; int* d_perm = nullptr; unsigned long long* d_spill = nullptr;
  auto run = [&]() -> lmx_status {
    LMX_HIP(hipMalloc((void**)&d_sim, (size_t)n * 4)); LMX_HIP(hipMalloc((void**)&d_tid, (size_t)n * 4)); LMX_HIP(hipMalloc((void**)&d_perm, (size_t)n * 4));
    LMX_HIP(hipMalloc((void**)&d_spill, (size_t)F2_MAX * 8));
    LMX_HIP(hipMemcpy(d_sim, similarity, (size_t)n * 4, hipMemcpyHostToDevice));
    LMX_HIP(hipMemcpy(d_tid, template_id, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_debug_block_sort(nullptr, d_sim, d_tid, n, d_perm, d_spill);
    LMX_HIP(hipGetLastError());
    LMX_HIP(hipDeviceSynchronize());
    LMX_HIP(hipMemcpy(perm, d_perm, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LMX_OK;
  };
  const lmx_status st = run();
  (void)hipFree(d_sim); (void)hipFree(d_tid); (void)hipFree(d_perm); (void)hipFree(d_spill);
  return st;
}
lmx_status lmx_debug_device_sort_perm_large(int32_t device, const float* similarity, const int32_t* template_id, int32_t n, int32_t* perm) {
  if (n < 0 || n > F2_LARGE_MAX || (n > 0 && (!similarity || !template_id || !perm))) { set_error("lmx_debug_device_sort_perm_large: invalid argument (n <= %d)", F2_LARGE_MAX); return LMX_ERR_INVALID_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  if (n == 0) return LMX_OK;
  LMX_HIP(hipSetDevice(device));
  float* d_sim = nullptr; int* d_tid = nullptr; int* d_perm = nullptr; uint8_t* d_ws = nullptr;
  auto run = [&]() -> lmx_status {
    LMX_HIP(hipMalloc((void**)&d_sim, (size_t)n * 4)); LMX_HIP(hipMalloc((void**)&d_tid, (size_t)n * 4)); LMX_HIP(hipMalloc((void**)&d_perm, (size_t)n * 4));
    LMX_HIP(hipMalloc((void**)&d_ws, f2_large_layout(F2_SIMILARITY).bytes));
    LMX_HIP(hipMemcpy(d_sim, similarity, (size_t)n * 4, hipMemcpyHostToDevice));
    LMX_HIP(hipMemcpy(d_tid, template_id, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_debug_block_sort_large(nullptr, d_sim, d_tid, n, d_perm, d_ws);
    LMX_HIP(hipGetLastError());
    LMX_HIP(hipDeviceSynchronize());
    LMX_HIP(hipMemcpy(perm, d_perm, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LMX_OK;
  };
  const lmx_status st = run();
  (void)hipFree(d_sim); (void)hipFree(d_tid); (void)hipFree(d_perm); (void)hipFree(d_ws);
  return st;
}
// the chain's kernels keep x, y as int16 and class_index as uint16 in LDS
static lmx_status check_hook_records(const char* what, const lmx_raw_match_t* records, size_t n_records) {
  for (size_t i = 0; i < n_records; ++i) {
    const lmx_raw_match_t& r = records[i];
    if (r.x < -32768 || r.x > 32767 || r.y < -32768 || r.y > 32767 || r.class_index < 0 || r.class_index > 65535) {
      set_error("%s: record %zu: x, y must fit an int16 and class_index a uint16", what, i);
      return LMX_ERR_INVALID_ARG;
    }
  }
  return LMX_OK;
}
// The large-frame kernels of a hook: every frame listed, one workspace part each (zeroed, as the LDS hooks zero their rows), then each
// part's output rows copied to the caller's [n_frames][F2_LARGE_MAX] rows.  p.out_counts is the hook's device count words.
static lmx_status debug_run_large(const F2Params& p, int32_t n_frames, F2Score score, bool classes, lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs,
                                  lmx_cluster_t* clusters, int32_t* cluster_class, int32_t* members) {
  const F2LargeLayout lay = f2_large_layout(score);
  const size_t F = (size_t)n_frames, N = (size_t)F2_LARGE_MAX;
  uint8_t* d_ws = nullptr;
  int32_t* d_frames = nullptr;
  auto run = [&]() -> lmx_status {
    LMX_HIP(hipMalloc((void**)&d_ws, F * lay.bytes));
    LMX_HIP(hipMalloc((void**)&d_frames, F * sizeof(int32_t)));
    LMX_HIP(hipMemset(d_ws, 0, F * lay.bytes));
    std::vector<int32_t> frames(F);
    for (size_t f = 0; f < F; ++f) frames[f] = (int32_t)f;
    LMX_HIP(hipMemcpy(d_frames, frames.data(), F * sizeof(int32_t), hipMemcpyHostToDevice));
    const F2LargeParams lp{p, d_frames, d_ws, lay};
    launch_f2_large(nullptr, lp, n_frames, score, classes);
    LMX_HIP(hipGetLastError());
    LMX_HIP(hipDeviceSynchronize());
    for (size_t f = 0; f < F; ++f) {
      const uint8_t* part = d_ws + f * lay.bytes;
      LMX_HIP(hipMemcpy(matches + f * N, part + lay.matches, N * sizeof(lmx_match_t), hipMemcpyDeviceToHost));
      LMX_HIP(hipMemcpy(clusters + f * N, part + lay.clusters, N * sizeof(lmx_cluster_t), hipMemcpyDeviceToHost));
      LMX_HIP(hipMemcpy(members + f * N, part + lay.members, N * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (cluster_class) LMX_HIP(hipMemcpy(cluster_class + f * N, part + lay.cluster_class, N * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (score != F2_SIMILARITY) LMX_HIP(hipMemcpy(diffs + f * N, part + lay.diffs, N * sizeof(lmx_depth_diff_t), hipMemcpyDeviceToHost));
      if (score == F2_DEPTH_NORMAL) LMX_HIP(hipMemcpy(ndiffs + f * N, part + lay.ndiffs, N * sizeof(lmx_normal_diff_t), hipMemcpyDeviceToHost));
    }
    return LMX_OK;
  };
  const lmx_status st = run();
  if (st != LMX_OK) (void)hipDeviceSynchronize();
  (void)hipFree(d_ws); (void)hipFree(d_frames);
  return st;
}
// The body of the cluster-chain hooks, their arguments checked: the whole device consumer chain (k_f2_finalize_cluster, as
// lmx_ctx_collect_clusters launches it) on a caller's record list.  The records become a raw-match slot of their own (16-dword header with
// [1] = n_records, cap = n_records); `sidecar(dev, p, w)` uploads the hook's side-car through `dev` and names it in the kernel's parameters,
// and says which records the walk takes; with a score the record walk runs on the stand-alone slot against the templates' resident scene
// (their mutex is the caller's to hold) in front of the chain.  The kernel's outputs and per-frame count words come back as written -- no
// host completion, so a test sees which path the kernel took; diffs / ndiffs [n_frames][2048] come back next to matches.
// large: the large-frame kernels on every frame, rows of F2_LARGE_MAX.
using HookAlloc = std::function<hipError_t(void**, size_t)>;
using HookSidecar = std::function<lmx_status(const HookAlloc&, F2Params&, DepthWalk&)>;
static lmx_status debug_chain(bool large, bool classes, F2Score score, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames, lmx_depth_templates* templates,
                              double no_value, const HookSidecar& sidecar, lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs, lmx_cluster_t* clusters,
                              int32_t* cluster_class, int32_t* members, uint32_t* counts) {
  const bool scored = score != F2_SIMILARITY, normals = score == F2_DEPTH_NORMAL;
  const size_t F = (size_t)n_frames, R = std::max<size_t>(n_records, 1), rows = F * F2_MAX;
  std::vector<void*> owned;   // every device buffer of this call
  const HookAlloc dev = [&](void** p, size_t bytes) -> hipError_t { const hipError_t e = hipMalloc(p, bytes); if (e == hipSuccess) owned.push_back(*p); return e; };
  auto zeroed = [&](void** p, size_t bytes) -> hipError_t { const hipError_t e = dev(p, bytes); return e == hipSuccess ? hipMemset(*p, 0, bytes) : e; };
  uint32_t hdr[16] = {0};
  hdr[1] = (uint32_t)n_records;
  uint32_t *d_hdr = nullptr, *d_counts = nullptr;
  lmx_raw_match_t* d_recs = nullptr;
  lmx_match_t* d_matches = nullptr;
  lmx_cluster_t* d_clusters = nullptr;
  int32_t *d_members = nullptr, *d_cluster_class = nullptr;
  uint8_t* d_scratch = nullptr;
  lmx_depth_diff_t *d_rec_diffs = nullptr, *d_diffs = nullptr, *d_diff_scratch = nullptr;
  lmx_normal_diff_t *d_rec_ndiffs = nullptr, *d_ndiffs = nullptr, *d_ndiff_scratch = nullptr;
  auto run = [&]() -> lmx_status {
    LMX_HIP(dev((void**)&d_hdr, sizeof(hdr)));
    LMX_HIP(dev((void**)&d_recs, R * sizeof(lmx_raw_match_t)));
    LMX_HIP(zeroed((void**)&d_matches, rows * sizeof(lmx_match_t)));
    LMX_HIP(zeroed((void**)&d_clusters, rows * sizeof(lmx_cluster_t)));
    LMX_HIP(zeroed((void**)&d_members, rows * sizeof(int32_t)));
    LMX_HIP(dev((void**)&d_counts, F * 4 * sizeof(uint32_t)));
    LMX_HIP(dev((void**)&d_scratch, rows * 32));
    LMX_HIP(hipMemcpy(d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice));
    if (n_records) LMX_HIP(hipMemcpy(d_recs, records, n_records * sizeof(lmx_raw_match_t), hipMemcpyHostToDevice));
    LMX_HIP(hipMemset(d_counts, 0xff, F * 4 * sizeof(uint32_t)));   // a frame the kernel did not report on stays recognisable
    F2Params p{};
    p.recs = d_recs; p.hdr = d_hdr; p.cap = (uint32_t)n_records; p.n_frames = n_frames;
    p.out_matches = d_matches; p.out_counts = d_counts; p.out_clusters = d_clusters; p.out_members = d_members; p.scratch = d_scratch;
    p.do_clusters = 1;
    DepthWalk w;
    w.recs = d_recs; w.n = (uint32_t)n_records;
    if (lmx_status ss = sidecar(dev, p, w)) return ss;
    if (classes) {
      LMX_HIP(zeroed((void**)&d_cluster_class, rows * sizeof(int32_t)));
      p.out_cluster_class = d_cluster_class;
    }
    if (scored) {
      LMX_HIP(dev((void**)&d_rec_diffs, R * sizeof(lmx_depth_diff_t)));
      LMX_HIP(zeroed((void**)&d_diffs, rows * sizeof(lmx_depth_diff_t)));
      LMX_HIP(dev((void**)&d_diff_scratch, 2 * rows * sizeof(lmx_depth_diff_t)));
      if (normals) {
        LMX_HIP(dev((void**)&d_rec_ndiffs, R * sizeof(lmx_normal_diff_t)));
        LMX_HIP(zeroed((void**)&d_ndiffs, rows * sizeof(lmx_normal_diff_t)));
        LMX_HIP(dev((void**)&d_ndiff_scratch, 2 * rows * sizeof(lmx_normal_diff_t)));
      }
      w.d_diffs = d_rec_diffs; w.d_ndiffs = d_rec_ndiffs;
      if (lmx_status ds = depth_launch_walk(templates, nullptr, w)) return ds;
      p.diffs = d_rec_diffs; p.out_diffs = d_diffs; p.diff_scratch = d_diff_scratch; p.no_value = no_value;
      p.ndiffs = d_rec_ndiffs; p.out_ndiffs = d_ndiffs; p.ndiff_scratch = d_ndiff_scratch;
    }
    if (large) {
      if (lmx_status ls = debug_run_large(p, n_frames, score, classes, matches, diffs, ndiffs, clusters, cluster_class, members)) return ls;
      LMX_HIP(hipMemcpy(counts, d_counts, F * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
      return LMX_OK;
    }
    launch_f2(nullptr, p, score, classes);
    LMX_HIP(hipGetLastError());
    LMX_HIP(hipDeviceSynchronize());
    if (scored) LMX_HIP(hipMemcpy(diffs, d_diffs, rows * sizeof(lmx_depth_diff_t), hipMemcpyDeviceToHost));
    if (normals) LMX_HIP(hipMemcpy(ndiffs, d_ndiffs, rows * sizeof(lmx_normal_diff_t), hipMemcpyDeviceToHost));
    LMX_HIP(hipMemcpy(matches, d_matches, rows * sizeof(lmx_match_t), hipMemcpyDeviceToHost));
    LMX_HIP(hipMemcpy(clusters, d_clusters, rows * sizeof(lmx_cluster_t), hipMemcpyDeviceToHost));
    if (classes) LMX_HIP(hipMemcpy(cluster_class, d_cluster_class, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    LMX_HIP(hipMemcpy(members, d_members, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    LMX_HIP(hipMemcpy(counts, d_counts, F * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return LMX_OK;
  };
  const lmx_status st = run();
  if (st != LMX_OK) (void)hipDeviceSynchronize();
  for (void* q : owned) (void)hipFree(q);
  return st;
}
// The un-classed hook: one side-car, no normal form.  templates != null: the depth-scored form, the templates' mutex is the caller's to hold.
static lmx_status debug_finalize_cluster(const char* what, int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames, lmx_depth_templates* templates,
                                         int32_t class_index, double no_value, const double* obj_origin_dists, const int32_t* rects, size_t n_templates,
                                         const lmx_cluster_params* params, lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_cluster_t* clusters,
                                         int32_t* members, uint32_t* counts, bool large = false /* the large-frame kernels on every frame, rows of F2_LARGE_MAX */) {
  if ((n_records && !records) || !obj_origin_dists || !rects || n_templates == 0 || !params || !matches || !clusters || !members || !counts) {
    set_error("%s: invalid argument", what);
    return LMX_ERR_INVALID_ARG;
  }
  if (n_frames < 1 || n_frames > 8) { set_error("%s: n_frames must be 1..8 (got %d)", what, n_frames); return LMX_ERR_INVALID_ARG; }
  if (n_records > ((size_t)1 << 24) || n_templates > ((size_t)1 << 24)) { set_error("%s: at most 2^24 records and templates", what); return LMX_ERR_INVALID_ARG; }
  if (params->vote_row_col_step <= 0) { set_error("vote_row_col_step must be positive"); return LMX_ERR_INVALID_ARG; }
  if (params->cluster_size_thresh < 0) { set_error("cluster_size_thresh must not be negative"); return LMX_ERR_INVALID_ARG; }
  if (lmx_status vs = check_vote_rings(obj_origin_dists, n_templates, params)) return vs;
  if (lmx_status rs = check_hook_records(what, records, n_records)) return rs;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  LMX_HIP(hipSetDevice(device));
  const HookSidecar sidecar = [&](const HookAlloc& dev, F2Params& p, DepthWalk& w) -> lmx_status {
    double* d_dists = nullptr;
    int32_t* d_rects = nullptr;
    LMX_HIP(dev((void**)&d_dists, n_templates * sizeof(double)));
    LMX_HIP(dev((void**)&d_rects, n_templates * 4 * sizeof(int32_t)));
    LMX_HIP(hipMemcpy(d_dists, obj_origin_dists, n_templates * sizeof(double), hipMemcpyHostToDevice));
    LMX_HIP(hipMemcpy(d_rects, rects, n_templates * 4 * sizeof(int32_t), hipMemcpyHostToDevice));
    p.dists = d_dists; p.rects = d_rects; p.n_templates = (uint32_t)n_templates;
    p.step = params->vote_row_col_step; p.size_thresh = params->cluster_size_thresh;
    p.radius_min = params->renderer_radius_min; p.radius_step = params->renderer_radius_step;
    w.class_index = class_index;
    return LMX_OK;
  };
  return lmx::guarded(what, [&]() -> lmx_status {   // the body allocates on the host
    return debug_chain(large, false, f2_score(templates != nullptr, false), records, n_records, n_frames, templates, no_value, sidecar, matches, diffs, nullptr, clusters,
                       nullptr, members, counts);
  });
}
lmx_status lmx_debug_device_finalize_cluster(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                             const double* obj_origin_dists, const int32_t* rects, size_t n_templates, const lmx_cluster_params* params,
                                             lmx_match_t* matches, lmx_cluster_t* clusters, int32_t* members, uint32_t* counts) {
  return debug_finalize_cluster("lmx_debug_device_finalize_cluster", device, records, n_records, n_frames, nullptr, -1, 0.0, obj_origin_dists, rects, n_templates, params, matches, nullptr, clusters,
                                members, counts);
}
lmx_status lmx_debug_device_finalize_cluster_large(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                   const double* obj_origin_dists, const int32_t* rects, size_t n_templates, const lmx_cluster_params* params,
                                                   lmx_match_t* matches, lmx_cluster_t* clusters, int32_t* members, uint32_t* counts) {
  return debug_finalize_cluster("lmx_debug_device_finalize_cluster_large", device, records, n_records, n_frames, nullptr, -1, 0.0, obj_origin_dists, rects, n_templates, params, matches,
                                nullptr, clusters, members, counts, true);
}
// The scored form of the same hook: `depth` (n_frames 16UC1 host frames) becomes the templates' resident scene, then the record walk and the
// depth-scored chain run on the stand-alone slot as lmx_ctx_collect_clusters_depth launches them.  No host completion.
static lmx_status debug_finalize_cluster_depth(const char* what, bool large, int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                               lmx_depth_templates* templates, const lmx_image* depth, int32_t class_index, double no_value,
                                               const double* obj_origin_dists, const int32_t* rects, size_t n_templates, const lmx_cluster_params* params,
                                               lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_cluster_t* clusters, int32_t* members, uint32_t* counts) {
  if (!templates || !depth || !diffs) { set_error("%s: invalid argument", what); return LMX_ERR_INVALID_ARG; }
  if (no_value != no_value) { set_error("%s: no_value is not a number", what); return LMX_ERR_INVALID_ARG; }
  if (n_frames < 1 || n_frames > 8) { set_error("%s: n_frames must be 1..8 (got %d)", what, n_frames); return LMX_ERR_INVALID_ARG; }
  if (depth_templates_scene(templates).device != device) { set_error("%s: the templates live on another device", what); return LMX_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(depth_templates_mutex(templates));   // held from the upload to the last launch: nobody replaces the scene between
  if (lmx_status st = depth_upload_scene(templates, depth, n_frames)) return st;
  return debug_finalize_cluster(what, device, records, n_records, n_frames, templates, class_index, no_value, obj_origin_dists, rects, n_templates, params, matches, diffs,
                                clusters, members, counts, large);
}
lmx_status lmx_debug_device_finalize_cluster_depth(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                   lmx_depth_templates* templates, const lmx_image* depth, int32_t class_index, double no_value,
                                                   const double* obj_origin_dists, const int32_t* rects, size_t n_templates, const lmx_cluster_params* params,
                                                   lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_cluster_t* clusters, int32_t* members, uint32_t* counts) {
  return debug_finalize_cluster_depth("lmx_debug_device_finalize_cluster_depth", false, device, records, n_records, n_frames, templates, depth, class_index, no_value, obj_origin_dists,
                                      rects, n_templates, params, matches, diffs, clusters, members, counts);
}
lmx_status lmx_debug_device_finalize_cluster_large_depth(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                         lmx_depth_templates* templates, const lmx_image* depth, int32_t class_index, double no_value,
                                                         const double* obj_origin_dists, const int32_t* rects, size_t n_templates, const lmx_cluster_params* params,
                                                         lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_cluster_t* clusters, int32_t* members, uint32_t* counts) {
  return debug_finalize_cluster_depth("lmx_debug_device_finalize_cluster_large_depth", true, device, records, n_records, n_frames, templates, depth, class_index, no_value,
                                      obj_origin_dists, rects, n_templates, params, matches, diffs, clusters, members, counts);
}
// The hook for the CLASSES forms: the records as a slot of their own, the classes' side-cars as the device table, then what
// lmx_ctx_collect_clusters_classes launches.  No host completion.
static lmx_status debug_finalize_cluster_classes(const char* what, bool large, int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                 const lmx_class_sidecar* classes, int32_t n_classes, const lmx_class_score* score, const lmx_image* depth,
                                                 lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs, lmx_cluster_t* clusters,
                                                 int32_t* cluster_class, int32_t* members, uint32_t* counts) {
  return lmx::guarded(what, [&]() -> lmx_status {
  const bool normals = score && score->normals != 0;
  if ((n_records && !records) || !classes || !matches || !clusters || !cluster_class || !members || !counts ||
      (score && (!score->templates || !score->class_base || !depth || !diffs)) || (normals && !ndiffs)) {
    set_error("%s: invalid argument", what);
    return LMX_ERR_INVALID_ARG;
  }
  if (n_classes < 1 || n_classes > F2_CLASSES) { set_error("%s: n_classes must be 1..%d (got %d)", what, F2_CLASSES, n_classes); return LMX_ERR_INVALID_ARG; }
  if (n_frames < 1 || n_frames > 8) { set_error("%s: n_frames must be 1..8 (got %d)", what, n_frames); return LMX_ERR_INVALID_ARG; }
  if (n_records > ((size_t)1 << 24)) { set_error("%s: at most 2^24 records", what); return LMX_ERR_INVALID_ARG; }
  for (int32_t k = 0; k < n_classes; ++k) {
    const lmx_class_sidecar& sc = classes[k];
    if (sc.n_templates == 0) continue;
    lmx_status vs = LMX_OK;
    if (!sc.obj_origin_dists || !sc.rects || sc.n_templates > ((size_t)1 << 24)) { set_error("invalid side-car (at most 2^24 templates)"); vs = LMX_ERR_INVALID_ARG; }
    else if (sc.params.vote_row_col_step <= 0) { set_error("vote_row_col_step must be positive"); vs = LMX_ERR_INVALID_ARG; }
    else if (sc.params.cluster_size_thresh < 0) { set_error("cluster_size_thresh must not be negative"); vs = LMX_ERR_INVALID_ARG; }
    else vs = check_vote_rings(sc.obj_origin_dists, sc.n_templates, &sc.params);
    if (vs != LMX_OK) { const std::string why = lmx_last_error(); set_error("%s: class %d: %s", what, k, why.c_str()); return vs; }
  }
  if (lmx_status rs = check_hook_records(what, records, n_records)) return rs;
  if (score) {
    if (score->no_value != score->no_value) { set_error("%s: no_value is not a number", what); return LMX_ERR_INVALID_ARG; }
    if (score->n_classes < 1 || score->n_classes > F2_CLASSES || score->class_base[0] != 0) { set_error("%s: class_base: n_classes 1..%d, class_base[0] = 0", what, F2_CLASSES); return LMX_ERR_INVALID_ARG; }
    for (int32_t k = 0; k < score->n_classes; ++k)
      if (score->class_base[k + 1] < score->class_base[k]) { set_error("%s: class_base must not decrease", what); return LMX_ERR_INVALID_ARG; }
    const DepthSceneInfo si = depth_templates_scene(score->templates);
    if (si.device != device) { set_error("%s: the templates live on another device", what); return LMX_ERR_INVALID_ARG; }
    if (score->class_base[score->n_classes] != si.count) { set_error("%s: class_base ends at %d but the object holds %d depth templates", what, score->class_base[score->n_classes], si.count); return LMX_ERR_INVALID_ARG; }
    if (normals && !si.normals) { set_error("%s: call lmx_depth_templates_enable_normals first", what); return LMX_ERR_INVALID_ARG; }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this library has no CPU path"); return LMX_ERR_NO_DEVICE; }
  LMX_HIP(hipSetDevice(device));
  std::unique_lock<std::mutex> lk;
  if (score) {   // held from the upload to the last launch: nobody replaces the scene between
    lk = std::unique_lock<std::mutex>(depth_templates_mutex(score->templates));
    if (lmx_status st = depth_upload_scene(score->templates, depth, n_frames)) return st;
  }
  const HookSidecar sidecar = [&](const HookAlloc& dev, F2Params& p, DepthWalk& w) -> lmx_status {
    F2Class* d_table = nullptr;
    LMX_HIP(dev((void**)&d_table, F2_CLASSES * sizeof(F2Class)));
    F2Class tab[F2_CLASSES] = {};
    for (int32_t k = 0; k < n_classes; ++k) {
      const lmx_class_sidecar& sc = classes[k];
      if (sc.n_templates == 0) continue;
      double* dd = nullptr;
      int32_t* dr = nullptr;
      LMX_HIP(dev((void**)&dd, sc.n_templates * sizeof(double)));
      LMX_HIP(dev((void**)&dr, sc.n_templates * 4 * sizeof(int32_t)));
      LMX_HIP(hipMemcpy(dd, sc.obj_origin_dists, sc.n_templates * sizeof(double), hipMemcpyHostToDevice));
      LMX_HIP(hipMemcpy(dr, sc.rects, sc.n_templates * 4 * sizeof(int32_t), hipMemcpyHostToDevice));
      tab[k] = F2Class{dd, dr, (uint32_t)sc.n_templates, sc.params.vote_row_col_step, sc.params.cluster_size_thresh, 0, sc.params.renderer_radius_min,
                       sc.params.renderer_radius_step};
    }
    LMX_HIP(hipMemcpy(d_table, tab, sizeof(tab), hipMemcpyHostToDevice));
    p.classes = d_table;
    if (score) {
      int32_t* d_class_base = nullptr;
      LMX_HIP(dev((void**)&d_class_base, (F2_CLASSES + 1) * sizeof(int32_t)));
      LMX_HIP(hipMemcpy(d_class_base, score->class_base, ((size_t)score->n_classes + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
      w.d_class_base = d_class_base; w.n_classes = score->n_classes;
    }
    return LMX_OK;
  };
  return debug_chain(large, true, f2_score(score != nullptr, normals), records, n_records, n_frames, score ? score->templates : nullptr, score ? score->no_value : 0.0,
                     sidecar, matches, diffs, ndiffs, clusters, cluster_class, members, counts);
  });
}
lmx_status lmx_debug_device_finalize_cluster_classes(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                     const lmx_class_sidecar* classes, int32_t n_classes, const lmx_class_score* score, const lmx_image* depth,
                                                     lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs, lmx_cluster_t* clusters,
                                                     int32_t* cluster_class, int32_t* members, uint32_t* counts) {
  return debug_finalize_cluster_classes("lmx_debug_device_finalize_cluster_classes", false, device, records, n_records, n_frames, classes, n_classes, score, depth, matches, diffs,
                                        ndiffs, clusters, cluster_class, members, counts);
}
lmx_status lmx_debug_device_finalize_cluster_large_classes(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                           const lmx_class_sidecar* classes, int32_t n_classes, const lmx_class_score* score,
                                                           const lmx_image* depth, lmx_match_t* matches, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs,
                                                           lmx_cluster_t* clusters, int32_t* cluster_class, int32_t* members, uint32_t* counts) {
  return debug_finalize_cluster_classes("lmx_debug_device_finalize_cluster_large_classes", true, device, records, n_records, n_frames, classes, n_classes, score, depth, matches,
                                        diffs, ndiffs, clusters, cluster_class, members, counts);
}
lmx_status lmx_debug_introsort_perm_score(const double* score, int32_t n, int32_t* perm) {
  if (n < 0 || (n > 0 && (!score || !perm))) { set_error("lmx_debug_introsort_perm_score: invalid argument"); return LMX_ERR_INVALID_ARG; }
  for (int32_t i = 0; i < n; ++i) perm[i] = i;
  lmx::sortemu::sort(perm, n, [&](int32_t a, int32_t b) { return score[a] > score[b]; });
  return LMX_OK;
}
}  // extern "C"
