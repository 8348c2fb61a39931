// The host bank, the per-level geometry and the tables the scoring and refinement kernels read (DeviceBankView), with the two pure functions
// that build them.  No HIP here: lmx_bank_tables.cpp is plain C++, lmx_ctx.cpp only uploads what it returns, and tests/test_bank_tables.py
// checks every table on the CPU through lmx_debug_bank_tables.  The table FORMATS are defined here and nowhere else.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <string>
#include <vector>

#include "lmx.h"

namespace lmx {

void set_error(const char* fmt, ...);

// ---- host bank (mirrors cv::linemod::Detector's template state) ---------------------------
struct ClassData {
  std::string id;
  int32_t n_pyramids = 0;
  std::vector<int32_t> templates;  // [n_pyramids * L*M][5], see TemplateRow
  std::vector<int32_t> features;   // [n][3] {x, y, label}
};

// One row of ClassData::templates: template k = l * M + m of pyramid t.
struct TemplateRow { int32_t width, height, level, feat_begin, feat_count; };
inline TemplateRow template_row(const ClassData& cd, int per /* L * M */, long t, int k) {
  const int32_t* p = &cd.templates[((size_t)t * per + k) * 5];
  return TemplateRow{p[0], p[1], p[2], p[3], p[4]};
}
inline const int32_t* template_features(const ClassData& cd, const TemplateRow& r) { return cd.features.data() + (size_t)r.feat_begin * 3; }

}  // namespace lmx

struct lmx_bank {
  std::vector<int32_t> T;
  std::vector<lmx_modality_desc> mods;
  std::map<std::string, lmx::ClassData> classes;  // std::map: upstream iterates classes in key order (A.10)
  std::vector<uint8_t> normal_lut;                // DepthNormal NORMAL_LUT[20][20][20] (one-hot labels), see include/lmx.h
  int32_t normal_lut_origin = 0;                  // LMX_LUT_*
  uint32_t lut_epoch = 0;                         // bumped by everything that replaces normal_lut (same size, new content)
  // lmx_bank_fingerprint hashes every template and feature (3.5 MB for 3000 templates: 2.8 ms), and lmx_ctx_acquire asks for it on every
  // request: remembered together with a signature of what it covered (element counts and lut_epoch: the API only appends templates or
  // replaces the table).  Copy-constructible on purpose (lmx_ctx_acquire keeps a private copy of the caller's bank).
  struct FingerprintCache {
    std::atomic<uint64_t> value{0}, signature{0};
    FingerprintCache() = default;
    FingerprintCache(const FingerprintCache& o) : value(o.value.load(std::memory_order_relaxed)), signature(o.signature.load(std::memory_order_relaxed)) {}
    FingerprintCache& operator=(const FingerprintCache& o) {
      value.store(o.value.load(std::memory_order_relaxed), std::memory_order_relaxed);
      signature.store(o.signature.load(std::memory_order_relaxed), std::memory_order_relaxed);
      return *this;
    }
  };
  mutable FingerprintCache fp_cache;
};

namespace lmx {

// ---- device-side geometry --------------------------------------------------------------------------------
constexpr int kMaxLevels = 4;
constexpr int kMaxModalities = 4;
constexpr int SB_GROUPS = 5, SB_BLOCK = 16, SB_MAX_BLOCKS = 6;   // scalar-block table of k_score_coarse_sb: <= 30 groups per template
constexpr int kFeatStride = 64;  // feature-table entries per (template, modality, level); upstream caps features at 63

struct LevelGeom {
  int32_t W, H;          // image size at this level
  int32_t T;             // sampling step
  int32_t Wc, Hc;        // W/T, H/T  (linear-memory "width"/"height")
  uint32_t cells;        // Wc*Hc      (length of one linear memory)
  uint32_t ori_stride;   // bytes per orientation block: T*T*cells + zero pad, multiple of 256
  uint32_t mod_stride;   // bytes per (frame, modality) at this level: 8*ori_stride + tail pad
  uint32_t zero_off;     // offset (within a modality block) of a run of >= cells+4096 zero bytes
  // nibble-packed memories of the coarsest level (two responses per byte), read by k_score_coarse:
  //   orientation o, byte i  =  elem(2i) | elem(2i + 1) << 4,  elem = the orientation's flat T*T*cells array, zero past its end.
  //   A feature whose first element index e0 is not a multiple of 8 starts in the middle of a dword: the kernel loads aligned
  //   dwords and funnel-shifts by 4 * (e0 & 7) bits with the neighbour lane's dword (v_alignbit_b32), so one copy serves
  //   every alignment.  Table entry = (dword index << 3) | (e0 & 7).
  uint32_t nib_ori_stride;    // bytes per orientation block incl. zero pad, multiple of 256
  uint32_t nib_mod_stride;    // bytes per (frame, modality): 8 * nib_ori_stride + tail pad
  uint32_t nib_zero_off;      // byte offset (multiple of 4) of a zero run (>= cells/2 + 2048 bytes) inside the block
  // finer levels keep NO response maps: only the spread image in linearize() order, one byte per cell.  k_refine derives the
  // 0..4 response of a feature's orientation from the spread byte with four nested bit masks (it touches a few hundred bytes
  // per candidate, so 8x fewer bytes are written and kept per frame than with materialised linear memories).
  uint32_t ls_stride;         // bytes per (frame, modality), multiple of 256
  uint32_t ls_zero_off;       // start of a zero run large enough for one patch
  // Banded form of that image (ls_bands > 0; Wc % 16 == 0, Wc >= 32).  View upstream's linear memories of one (frame, modality)
  // as ONE matrix of R = T*T*Hc rows x Wc columns (row = grid * Hc + cell row; flat index = row * Wc + column, a column past
  // Wc continues in the next row exactly as in the flat array).  Band k keeps columns 16k .. 16k+31 of every row in 32 bytes:
  //     byte (k * ls_band_stride + (row + 1) * 32 + c)  =  flat element row * Wc + 16k + c,      0 <= c < 32,
  // so every cell is stored twice and the 16 x 16 patch k_refine gathers for a feature (any origin) is 16 consecutive 32-byte
  // rows of one band: 4-5 cache lines instead of 16-17 (the gathers miss L2; round 2 measured the flat form at 5.4 TB/s of HBM
  // fetches, 730 lines per candidate).  Row 0 of a band is slack for the writer, rows R+1 .. R+16 stay zero.
  uint32_t ls_bands;          // 0: flat form
  uint32_t ls_band_stride;    // bytes per band: (R + 17) * 32
};

// Fine-level feature table entry (refinement needs x,y for upstream's out-of-bounds skip).
struct FeatEntry {
  uint32_t off;    // finer levels: label << 29 | (grid_row*cells + lm_index) into the linearised spread image
  int16_t x, y;
};

struct TemplateInfo {    // per shard-local template g
  int32_t class_index;
  int32_t template_id;   // id within its class (global, not shard-local)
  int32_t class_slot;    // unused on device; slot is taken from the per-call class_slot table
  int32_t pad;
};

struct TemplateLevelInfo {  // per (g, level)
  int32_t width, height;    // of template l*M+0 (upstream uses tp[start] for the refinement clamp)
  int32_t nf_total;         // sum over modalities of features.size() at this level
  int32_t positions;        // template_positions at this level (only the coarsest is used)
};

struct ScoreInfo {           // per shard-local template: everything k_score_coarse_u8 needs, one 16-byte scalar load
  int32_t positions;        // template_positions at the coarsest level
  int32_t nf_total;         // features at the coarsest level, all modalities
  int32_t class_index;
  uint32_t groups;          // fast groups | all groups << 8 of the unified table row | blocks of the scalar-block row << 16
};

// ---- the two pure functions ------------------------------------------------------------------------------
// Geometry of every pyramid level of `bank` for width x height frames into geom[bank.T.size()]; ls_flat (LMX_LS_FLAT) keeps every
// finer level's spread image flat.  LMX_ERR_SHAPE / LMX_ERR_INVALID_ARG with the error text set when upstream would assert.
lmx_status build_geometry(const lmx_bank& bank, int width, int height, bool ls_flat, LevelGeom* geom);

// The contiguous template ids of one class that shard `rank` of `world` holds.
inline void shard_range(long n_pyramids, int rank, int world, long* begin, long* end) {
  *begin = (rank * n_pyramids) / world; *end = ((rank + 1) * n_pyramids) / world;
}
// Placements of a width x height template on level g's grid of cells (upstream matchClass: the template's span in cells must fit).
inline int32_t template_positions(const LevelGeom& g, int width, int height) {
  const int wf = (width - 1) / g.T + 1, hf = (height - 1) / g.T + 1;
  return (int32_t)std::max<long>(0, std::min<long>((long)(g.Hc - hf) * g.Wc + (g.Wc - wf) + 1, (long)g.cells));
}

// What DeviceBankView's pointers of the same names point at (lmx_internal.hpp has the layouts), as host vectors.
struct BankTables {
  std::vector<TemplateInfo> info;
  std::vector<TemplateLevelInfo> linfo;
  std::vector<uint32_t> coarse_off, coarse_uni, coarse_blk;
  std::vector<ScoreInfo> sinfo;
  std::vector<FeatEntry> feat;
  std::vector<uint8_t> feat_count;
  std::vector<std::string> class_names;    // in class_index order
  int32_t G = 0, nf_max_coarse = 0, uni_ok = 0;
  uint32_t uni_mod_block_bytes = 0;
};
void build_bank_tables(const lmx_bank& bank, const LevelGeom* geom, int max_batch, int shard_rank, int shard_world, BankTables* out);

}  // namespace lmx
