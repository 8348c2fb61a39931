// liblmx.so, the per-level geometry of a context and the tables its scoring and refinement kernels read, built from the host bank alone:
// plain C++ without a device call, so that tests/test_bank_tables.py can check every byte on the CPU (lmx_debug_bank_tables).  Each address
// formula and each table encoding is written once, here.

#include <algorithm>

#include "lmx_bank_tables.hpp"

namespace lmx {
namespace {

uint32_t round_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }

// accessLinearMemory: which of the T*T grids a feature falls into, and its flat element index inside one orientation's [T*T][cells] matrix
uint32_t grid_of(const LevelGeom& g, int x, int y) { return (uint32_t)((y % g.T) * g.T + (x % g.T)); }
uint32_t linear_index(const LevelGeom& g, int x, int y) { return grid_of(g, x, y) * g.cells + (uint32_t)(y / g.T) * g.Wc + (uint32_t)(x / g.T); }

// Coarsest level (scoring): (aligned dword index << 3) | nibble shift into the nibble-packed memories of one modality
uint32_t nibble_entry(const LevelGeom& g, int label, uint32_t e0) { return ((((uint32_t)label * g.nib_ori_stride) >> 2) + (e0 >> 3)) << 3 | (e0 & 7u); }
uint32_t nibble_zero_entry(const LevelGeom& g) { return (g.nib_zero_off >> 2) << 3; }   // the zero run, shift 0
// Finer levels (refinement): label in the top 3 bits; below it the flat element index into the linearised spread image, or, for a banded
// image, the row and the column of the matrix (label:3 | row:17 | column:12; build_geometry checked the ranges)
uint32_t feat_entry_off(const LevelGeom& g, int label, int x, int y) {
  if (g.ls_bands) return ((uint32_t)label << 29) | (grid_of(g, x, y) * g.Hc + (uint32_t)(y / g.T)) << 12 | (uint32_t)(x / g.T);
  return ((uint32_t)label << 29) | linear_index(g, x, y);
}
// Final form of a unified-table entry: byte offset (< 2^27, see uni_ok) | funnel-shift bits (4 * nibble) << 27, one scalar instruction each
uint32_t uni_final(uint32_t e) { return ((e >> 3) << 2) | ((e & 7u) * 4u) << 27; }

// True when every feature of pyramid level l packs into the banded table entry.
bool level_features_pack(const lmx_bank& b, int l, const LevelGeom& g) {
  const int M = (int)b.mods.size(), per = (int)b.T.size() * M;
  for (const auto& kv : b.classes) {
    const ClassData& cd = kv.second;
    for (long t = 0; t < cd.n_pyramids; ++t)
      for (int m = 0; m < M; ++m) {
        const TemplateRow tm = template_row(cd, per, t, l * M + m);
        const int32_t* ft = template_features(cd, tm);
        for (int f = 0; f < tm.feat_count; ++f, ft += 3) {
          if (ft[0] < 0 || ft[1] < 0 || ft[0] / g.T >= 4096) return false;
          if ((long)grid_of(g, ft[0], ft[1]) * g.Hc + ft[1] / g.T >= (1L << 17)) return false;
        }
      }
  }
  return true;
}

// The coarsest level's rows of ONE template for k_score_coarse_u8 (row[kFeatStride]) and k_score_coarse_sb (brow[SB_MAX_BLOCKS * SB_BLOCK]),
// from its modalities' coarse_off rows.  The entries, moved to their modality's block, are taken from the modalities three at a time (round
// robin) and sorted into classes by nibble shift (entry & 7).  Triples of ONE class come first ("fast" groups: the kernel sums the three dwords
// before the funnel shift), taken round robin over the classes, from class 0, so that the modalities stay mixed; both rows hold them in that
// order.  Then the leftovers (< 3 per class) in class order: the unified row packs them into mixed groups and pads the last one with zero-run
// entries, the block row gives each class a group of its own, padded.  row[63] = fast groups | all groups << 8.  A block is 5 groups x 3 byte
// offsets and one word: the groups' shifts (5 bits each) | the real features consumed up to the block's end << 25.
// Returns ScoreInfo::groups; *blocks_fit = false when the groups overflow the block row (cannot happen for <= 63 features: <= 21 + 8 groups).
uint32_t encode_coarse_rows(const LevelGeom& g, int M, const uint8_t* cnt, const uint32_t* offs, uint32_t uni_block, std::vector<uint32_t> (&cls)[8],
                            uint32_t* row, uint32_t* brow, bool* blocks_fit) {
  int next[kMaxModalities] = {0, 0, 0, 0};
  for (std::vector<uint32_t>& v : cls) v.clear();
  for (bool any = true; any;) {
    any = false;
    for (int m = 0; m < M; ++m)
      for (int u = 0; u < 3 && next[m] < cnt[m]; ++u, any = true) {
        const uint32_t e = offs[(size_t)m * kFeatStride + next[m]++] + ((((uint64_t)m * uni_block) >> 2) << 3);
        cls[e & 7u].push_back(e);
      }
  }
  const uint32_t zero_entry = g.nib_zero_off & ~3u;   // byte offset of the zero run (modality 0's block; any shift reads zeros)
  std::fill(brow, brow + SB_BLOCK * SB_MAX_BLOCKS, zero_entry);
  int n = 0, n_grps = 0;
  uint32_t meta = 0, consumed = 0;
  auto put_group = [&](int k, const uint32_t* e, int real) {   // `real` entries of class k into both rows; the block row pads the group
    for (int u = 0; u < real; ++u) row[n++] = e[u];
    if (n_grps < SB_GROUPS * SB_MAX_BLOCKS) {
      const int q = n_grps % SB_GROUPS;
      uint32_t* blk = brow + (size_t)(n_grps / SB_GROUPS) * SB_BLOCK;
      for (int u = 0; u < real; ++u) blk[3 * q + u] = (e[u] >> 3) << 2;
      meta = (q ? meta : 0u) | ((uint32_t)k * 4u) << (5 * q);
      consumed += (uint32_t)real;
      blk[SB_BLOCK - 1] = meta | consumed << 25;
    }
    ++n_grps;
  };
  size_t taken[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int n_fast = 0;
  for (bool any = true; any;) {
    any = false;
    for (int k = 0; k < 8; ++k)
      if (cls[k].size() - taken[k] >= 3) {
        put_group(k, &cls[k][taken[k]], 3);
        taken[k] += 3; ++n_fast; any = true;
      }
  }
  for (int k = 0; k < 8; ++k)
    if (taken[k] < cls[k].size()) put_group(k, &cls[k][taken[k]], (int)(cls[k].size() - taken[k]));
  for (int i = 0; i < kFeatStride - 1; ++i) row[i] = uni_final(row[i]);
  row[kFeatStride - 1] = (uint32_t)n_fast | ((uint32_t)((n + 2) / 3) << 8);
  const int n_blocks = (n_grps + SB_GROUPS - 1) / SB_GROUPS;
  *blocks_fit = n_blocks <= SB_MAX_BLOCKS;
  if (!*blocks_fit) std::fill(brow, brow + SB_BLOCK * SB_MAX_BLOCKS, 0u);
  return row[kFeatStride - 1] | (*blocks_fit ? (uint32_t)n_blocks << 16 : 0u);
}

}  // namespace

lmx_status build_geometry(const lmx_bank& bank, int W, int H, bool ls_flat, LevelGeom* geom) {
  const int L = (int)bank.T.size();
  for (int l = 0; l < L; ++l) {
    if (l > 0) { W /= 2; H /= 2; }
    const int T = bank.T[l];
    if (T < 1 || T > 16) { set_error("T=%d at level %d unsupported (1..16)", T, l); return LMX_ERR_INVALID_ARG; }
    if (W <= 0 || H <= 0 || W % T != 0 || H % T != 0) { set_error("image size %dx%d at pyramid level %d is not a multiple of T=%d (upstream linearize CV_Assert)", W, H, l, T); return LMX_ERR_SHAPE; }
    // the fused pyrDown reflects at most two pixels across a border
    if (l + 1 < L && (W < 4 || H < 4)) { set_error("image size %dx%d at pyramid level %d is too small to be downsampled again", W, H, l); return LMX_ERR_SHAPE; }
    if (((long)W * H) % 16 != 0) { set_error("rows*cols = %ld at level %d is not a multiple of 16 (upstream computeResponseMaps CV_Assert)", (long)W * H, l); return LMX_ERR_SHAPE; }
    LevelGeom& g = geom[l];
    g.W = W; g.H = H; g.T = T; g.Wc = W / T; g.Hc = H / T;
    g.cells = (uint32_t)g.Wc * g.Hc;
    const uint32_t pad = g.cells + std::max<uint32_t>(16u * g.Wc + 64u, 2048u);
    g.ori_stride = round_up((uint32_t)T * T * g.cells + pad, 256);
    g.mod_stride = 8 * g.ori_stride + 8192;
    g.zero_off = (uint32_t)T * T * g.cells;
    const uint32_t nib_bytes = ((uint32_t)T * T * g.cells + 1) / 2;
    g.nib_ori_stride = round_up(nib_bytes + g.cells / 2 + 2048 + 64, 256);
    g.nib_mod_stride = 8 * g.nib_ori_stride + 8192;
    g.nib_zero_off = round_up(nib_bytes + 32, 4);
    g.ls_zero_off = (uint32_t)T * T * g.cells;
    g.ls_stride = round_up(g.ls_zero_off + pad, 256);
    g.ls_bands = 0; g.ls_band_stride = 0;
    if (l < L - 1 && g.Wc % 16 == 0 && g.Wc >= 32 && !ls_flat) {
      const uint32_t rows = (uint32_t)T * T * g.Hc;
      if (rows < (1u << 17) && g.Wc < 4096 && level_features_pack(bank, l, g)) {
        g.ls_bands = (uint32_t)g.Wc / 16;
        g.ls_band_stride = (rows + 17) * 32;
        g.ls_zero_off = (rows + 1) * 32;          // band 0, the 16 never-written rows behind the image
        g.ls_stride = round_up(g.ls_bands * g.ls_band_stride, 256);
      }
    }
  }
  return LMX_OK;
}

void build_bank_tables(const lmx_bank& b, const LevelGeom* geom, int max_batch, int shard_rank, int shard_world, BankTables* out) {
  const int L = (int)b.T.size(), M = (int)b.mods.size(), per = L * M, world = std::max(1, shard_world);
  const LevelGeom& gc = geom[L - 1];
  const uint32_t uni_block = (uint32_t)max_batch * gc.nib_mod_stride;
  BankTables& o = *out;
  o = BankTables{};
  size_t G = 0;
  for (const auto& kv : b.classes) {
    long begin, end;
    shard_range(kv.second.n_pyramids, shard_rank, world, &begin, &end);
    G += (size_t)(end - begin);
  }
  // every table has a fixed row per template: sized once, written in place.  A template that is not uni_ok keeps what its rows get here:
  // un-encoded zero-run entries in coarse_uni, zeros in coarse_blk
  o.info.resize(G); o.linfo.resize(G * L); o.sinfo.resize(G);
  o.coarse_off.assign(G * M * kFeatStride, nibble_zero_entry(gc));
  o.coarse_uni.assign(G * kFeatStride, nibble_zero_entry(gc));
  o.coarse_blk.assign(G * SB_BLOCK * SB_MAX_BLOCKS, 0u);
  o.feat.resize((size_t)L * G * M * kFeatStride); o.feat_count.resize((size_t)L * G * M);
  bool uni_ok = true;
  std::vector<uint32_t> cls[8];
  int ci = 0, nf_max = 0;
  size_t gi = 0;
  for (const auto& kv : b.classes) {
    const ClassData& cd = kv.second;
    o.class_names.push_back(kv.first);
    long begin, end;
    shard_range(cd.n_pyramids, shard_rank, world, &begin, &end);
    for (long t = begin; t < end; ++t, ++gi) {
      o.info[gi] = TemplateInfo{ci, (int32_t)t, 0, 0};
      for (int l = 0; l < L; ++l) {
        const LevelGeom& g = geom[l];
        const bool coarsest = l == L - 1;
        const TemplateRow t0 = template_row(cd, per, t, l * M);
        TemplateLevelInfo li{t0.width, t0.height, 0, template_positions(g, t0.width, t0.height)};
        uint8_t* cnt = &o.feat_count[((size_t)l * G + gi) * M];
        uint32_t* offs = &o.coarse_off[gi * M * kFeatStride];
        for (int m = 0; m < M; ++m) {
          const TemplateRow tm = template_row(cd, per, t, l * M + m);
          const int fc = tm.feat_count;
          li.nf_total += fc;
          cnt[m] = (uint8_t)fc;
          FeatEntry* ent = &o.feat[(((size_t)l * G + gi) * M + m) * kFeatStride];
          const int32_t* ft = template_features(cd, tm);
          for (int f = 0; f < fc; ++f, ft += 3) {
            const int x = ft[0], y = ft[1], label = ft[2];
            ent[f] = FeatEntry{feat_entry_off(g, label, x, y), (int16_t)x, (int16_t)y};
            // upstream similarity() skips out-of-image features: they keep the zero run
            if (coarsest && x < g.W && y < g.H) offs[(size_t)m * kFeatStride + f] = nibble_entry(g, label, linear_index(g, x, y));
          }
          for (int f = fc; f < kFeatStride; ++f) ent[f] = FeatEntry{g.ls_zero_off, 0, 0};
          ent[kFeatStride - 1].y = (int16_t)fc;   // entry 63 is always padding (<= 63 features): k_refine reads the row's feature count from it
          if (coarsest) nf_max = std::max(nf_max, fc);
        }
        o.linfo[gi * L + l] = li;
        if (!coarsest) continue;
        uint32_t groups = 0;
        bool fit = false;
        if (li.nf_total <= kFeatStride - 1)
          groups = encode_coarse_rows(g, M, cnt, offs, uni_block, cls, &o.coarse_uni[gi * kFeatStride], &o.coarse_blk[gi * SB_BLOCK * SB_MAX_BLOCKS], &fit);
        uni_ok = uni_ok && fit;
        o.sinfo[gi] = ScoreInfo{li.positions, li.nf_total, ci, groups};
      }
    }
    ++ci;
  }
  o.G = (int32_t)G; o.nf_max_coarse = nf_max;
  o.uni_ok = (uni_ok && (uint64_t)M * uni_block + gc.nib_mod_stride < (1u << 27)) ? 1 : 0;  // byte offsets inside one frame's block
  o.uni_mod_block_bytes = uni_block;
}

}  // namespace lmx
