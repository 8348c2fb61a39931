// Candidate lists of the mesh trainer's device path (lmx_bank_train_mesh_opts with LMX_TRAIN_CANDIDATES_DEVICE, include/lmx.h): the per-pixel
// half of extractTemplate on one window -- which pixels are candidates, in raster order, and the few scalars the ranking needs -- shared by
// the HIP kernel (lmx_train_cand.hip, k_train_candidates) and by plain CPU builds (LMX_TC_HOST, set for any compiler but hipcc: tests/cpp/
// train_cand_host.cpp).  The host keeps the sequential rest (lmx_train_select.hpp: rank_select_color / rank_select_depth).
//
// ColorGradient.  Pixel (x, y) of the window is a candidate iff
//     (no mask  or  mask > min3x3(mask), the 3x3 minimum with BORDER_REPLICATE on the window: mask - erode3(mask) saturating, non-zero)
//     and  q > 0  and  mag > strong_threshold * strong_threshold (the float product extract_color forms);       score = mag.
// DepthNormal.  local = the 5x5 replicate-clamped minimum of the mask is non-zero (= erode3 twice; true everywhere without a mask).
//     candidate iff  local  and  q one-hot (not 0, not 255)  and  dist_label(q) >= extract_threshold;           score = (float)dist,
//     the RAW integer distance; the header carries label_counts[8] and area = #{local} (w * h without a mask) for the host's
//     score /= (float)label_counts[label] and its first selection distance.
//
// Chessboard distance without eight distance images: the byte temp = local ? q : 0 holds the eight label planes as bit-planes (255 is
// non-zero in every plane, as in extract_depth).  One step is a 3x3 bitwise AND with everything outside the window read as 0xFF; after s
// steps a bit is still set iff its plane's distance to the nearest zero pixel exceeds s.  So a pixel's distance for its own label is the
// number of the step that clears its bit, and a bit that survives max(w, h) steps has no zero pixel in its plane at all: the host code's
// (float)(1 << 28).  The step is separable and runs on four pixels per dword (and_step_rows).  The step counter is an int: distances
// above 255 are ordinary (a 3 x 520 strip with one zero pixel).
//
// Window image: rows of row_dwords(w) dwords, pixel x of a row in byte x & 3 of dword x >> 2; the bytes of a row's last dword at x >= w
// ("padding") are kept at 0xFF, which is what "outside the window" reads as.
//
// List: records of 8 bytes in raster order {x | y << 14 | label << 28, float score}, coordinates window-relative (sides <= 16384); a label
// that is no single bit decodes as -1 (label_of).  ListHeader: n_cands, area, label_counts[8], status, offset (in records, into the
// batch's record buffer).  status != 0: the window was not processed (ST_TOO_LARGE) or its list did not fit the buffer (ST_OVERFLOW);
// the view is then trained by the pack-and-host path.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(LMX_TC_HOST)
#define LMX_TC_HOST   // a plain C++ compiler: the CPU build
#endif
#ifdef LMX_TC_HOST
#include <vector>
#define LMX_TC_FN inline
#else
#define LMX_TC_FN __host__ __device__ __forceinline__
#endif

namespace lmx {
namespace train_cand {

constexpr int kMaxWindowDwords = 16384;   // one window image in LDS (64 KiB, rows padded to whole dwords); the kernel keeps two
constexpr int kMaxWindowPixels = 4 * kMaxWindowDwords;       // what such an image holds at most; every window of w * h <= 40000 fits (sides <= 16384)
constexpr int kMaxBitWords = kMaxWindowPixels / 32;          // one bit per pixel, flat index y * w + x
constexpr uint32_t kNoZeroDistance = 1u << 28;               // extract_depth's distance where a plane has no zero pixel
constexpr uint32_t ST_TOO_LARGE = 1, ST_OVERFLOW = 2;

struct Record { uint32_t xyl; float score; };
struct ListHeader { uint32_t n_cands, area, label_counts[8], status, offset, reserved[4]; };   // 64 bytes
static_assert(sizeof(Record) == 8 && sizeof(ListHeader) == 64, "the formats the host decodes");

LMX_TC_FN uint32_t pack_xyl(int x, int y, int label) { return (uint32_t)x | (uint32_t)y << 14 | ((uint32_t)label & 15u) << 28; }
LMX_TC_FN int rec_x(uint32_t v) { return (int)(v & 0x3fffu); }
LMX_TC_FN int rec_y(uint32_t v) { return (int)(v >> 14 & 0x3fffu); }
LMX_TC_FN int rec_label(uint32_t v) { const int l = (int)(v >> 28); return l > 7 ? -1 : l; }

// getLabel(): one-hot byte -> bin, anything else -1
LMX_TC_FN int label_of(uint32_t q) {
  if (q == 0 || (q & (q - 1)) != 0 || q > 128) return -1;
  int k = 0;
  while ((q >> k) != 1u) ++k;
  return k;
}

LMX_TC_FN int row_dwords(int w) { return (w + 3) >> 2; }
// the windows the device path takes: the padded image fits kMaxWindowDwords
LMX_TC_FN bool window_fits(int w, int h) { return w >= 1 && h >= 1 && w <= 16384 && h <= 16384 && (int64_t)row_dwords(w) * h <= kMaxWindowDwords; }
// the padding bytes of a row's last dword
LMX_TC_FN uint32_t pad_mask(int w) { return (w & 3) ? 0xffffffffu << (8 * (w & 3)) : 0u; }
// per byte: 0xFF where the byte is non-zero
LMX_TC_FN uint32_t nonzero_bytes(uint32_t v) {
  uint32_t t = v | v >> 4;
  t |= t >> 2;
  t |= t >> 1;
  return (t & 0x01010101u) * 0xffu;
}
// bit j: byte j is non-zero
LMX_TC_FN uint32_t nonzero_nibble(uint32_t v) {
  const uint32_t t = nonzero_bytes(v) & 0x08040201u;
  return (t | t >> 8 | t >> 16 | t >> 24) & 15u;
}
// bit j: byte j is a single bit (a label, not 0 and not 255)
LMX_TC_FN uint32_t onehot_nibble(uint32_t v) {
  uint32_t out = 0;
  for (int j = 0; j < 4; ++j) {
    const uint32_t q = v >> (8 * j) & 255u;
    out |= (uint32_t)(q != 0 && (q & (q - 1)) == 0) << j;
  }
  return out;
}
// horizontal part of the step: each byte ANDed with its two neighbours; l / r are the dwords to the left and right (0xFFFFFFFF outside)
LMX_TC_FN uint32_t hand3(uint32_t l, uint32_t c, uint32_t r) { return c & (c << 8 | l >> 24) & (c >> 8 | r << 24); }
LMX_TC_FN uint32_t hrow(const uint32_t* img, int ws, int h, int r, int c) {
  if (r < 0 || r >= h) return 0xffffffffu;
  const uint32_t* row = img + (size_t)r * ws;
  return hand3(c > 0 ? row[c - 1] : 0xffffffffu, row[c], c + 1 < ws ? row[c + 1] : 0xffffffffu);
}
// One AND step of dword column c, rows [r0, r1): out = the 3x3 AND of in (outside = 0xFF), padding bytes back at 0xFF.  on_dword(r, in, out)
// sees every dword whose value changed.  -> the OR of the outputs' window bytes (0: this part of the image is all zero).
constexpr int kStepRows = 8;   // rows per work item: 3 (R + 2) reads for R outputs
template <class F>
LMX_TC_FN uint32_t and_step_rows(const uint32_t* in, uint32_t* out, int ws, int h, uint32_t pad, int c, int r0, int r1, F&& on_dword) {
  const uint32_t pm = c == ws - 1 ? pad : 0u;
  uint32_t up = hrow(in, ws, h, r0 - 1, c), mid = hrow(in, ws, h, r0, c), any = 0;
  for (int r = r0; r < r1; ++r) {
    const uint32_t dn = hrow(in, ws, h, r + 1, c);
    const uint32_t o = (up & mid & dn) | pm, i = in[(size_t)r * ws + c];
    out[(size_t)r * ws + c] = o;
    any |= o & ~pm;
    if (o != i) on_dword(r, i, o);
    up = mid; mid = dn;
  }
  return any;
}
// bits [i, i + 4) of a flat bitmap
LMX_TC_FN uint32_t bits4(const uint32_t* bits, uint32_t i) {
  const uint32_t wd = i >> 5, sh = i & 31;
  uint32_t v = bits[wd] >> sh;
  if (sh > 28) v |= bits[wd + 1] << (32 - sh);
  return v & 15u;
}
LMX_TC_FN bool color_candidate(bool has_mask, uint32_t m, uint32_t m_min3x3, uint32_t q, float mag, float threshold_sq) {
  return (!has_mask || m > m_min3x3) && q > 0 && mag > threshold_sq;
}
LMX_TC_FN float color_threshold_sq(float strong_threshold) { return strong_threshold * strong_threshold; }
LMX_TC_FN int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

#ifdef LMX_TC_HOST
// ---- the whole window on the CPU, in the kernel's phases (one "thread"): what tests/cpp/train_cand_host.cpp runs -----------------------
struct WindowList {
  ListHeader header;
  std::vector<Record> records;
};

inline void color_window(const uint8_t* label, const float* mag, const uint8_t* mask /* null: none */, int h, int w, float strong_threshold, WindowList* out) {
  out->header = ListHeader();
  out->records.clear();
  if (!window_fits(w, h)) { out->header.status = ST_TOO_LARGE; return; }
  const float thr = color_threshold_sq(strong_threshold);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      uint32_t mn = 255;
      if (mask)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t v = mask[(size_t)clampi(y + dy, 0, h - 1) * w + clampi(x + dx, 0, w - 1)];
            mn = v < mn ? v : mn;
          }
      if (color_candidate(mask != nullptr, mask ? mask[i] : 0, mn, label[i], mag[i], thr)) out->records.push_back(Record{pack_xyl(x, y, label_of(label[i])), mag[i]});
    }
  out->header.n_cands = (uint32_t)out->records.size();
}

inline void depth_window(const uint8_t* label, const uint8_t* mask /* null: none */, int h, int w, int extract_threshold, WindowList* out) {
  out->header = ListHeader();
  out->records.clear();
  if (!window_fits(w, h)) { out->header.status = ST_TOO_LARGE; return; }
  const int ws = row_dwords(w);
  const uint32_t pad = pad_mask(w);
  std::vector<uint32_t> a((size_t)ws * h), b((size_t)ws * h), bits(((size_t)w * h + 31) / 32 + 1, 0u), pre(bits.size(), 0u);
  auto load = [&](const uint8_t* src, int r, int c, bool as_mask) {
    uint32_t v = 0;
    for (int j = 0; j < 4; ++j) {
      const int x = 4 * c + j;
      if (x < w) v |= (uint32_t)(as_mask ? (src[(size_t)r * w + x] ? 255 : 0) : src[(size_t)r * w + x]) << (8 * j);
    }
    return v;
  };
  auto step_all = [&](const std::vector<uint32_t>& in, std::vector<uint32_t>& o, auto&& f) {
    uint32_t any = 0;
    for (int r0 = 0; r0 < h; r0 += kStepRows)
      for (int c = 0; c < ws; ++c) {
        auto g = [&](int r, uint32_t i, uint32_t ov) { f(r, c, i, ov); };
        any |= and_step_rows(in.data(), o.data(), ws, h, pad, c, r0, r0 + kStepRows < h ? r0 + kStepRows : h, g);
      }
    return any;
  };
  // local: two erosions of mask != 0
  if (mask) {
    for (int r = 0; r < h; ++r)
      for (int c = 0; c < ws; ++c) a[(size_t)r * ws + c] = load(mask, r, c, true) | (c == ws - 1 ? pad : 0u);
    step_all(a, b, [&](int, int, uint32_t, uint32_t) {});
    step_all(b, a, [&](int, int, uint32_t, uint32_t) {});
  }
  uint32_t area = 0;
  for (int r = 0; r < h; ++r)
    for (int c = 0; c < ws; ++c) {
      const uint32_t pm = c == ws - 1 ? pad : 0u;
      const uint32_t loc = mask ? a[(size_t)r * ws + c] & ~pm : ~pm;
      const uint32_t t = load(label, r, c, false) & loc;
      area += (uint32_t)__builtin_popcount(loc) / 8;
      a[(size_t)r * ws + c] = t | pm;
      const uint32_t oh = onehot_nibble(t), i = (uint32_t)r * w + 4 * c;
      for (int j = 0; j < 4; ++j)
        if (oh >> j & 1) bits[(i + j) >> 5] |= 1u << ((i + j) & 31);
    }
  out->header.area = area;
  bool built = false;
  const bool thr_reachable = (int64_t)extract_threshold <= (int64_t)kNoZeroDistance;
  auto build = [&](const std::vector<uint32_t>& in) {
    uint32_t n = 0;
    for (int r = 0; r < h; ++r)
      for (int c = 0; c < ws; ++c) {
        const uint32_t v = in[(size_t)r * ws + c], i = (uint32_t)r * w + 4 * c;
        const uint32_t nz = thr_reachable ? nonzero_nibble(v) : 0u;
        for (int j = 0; j < 4 && 4 * c + j < w; ++j) {
          uint32_t& wd = bits[(i + j) >> 5];
          const uint32_t bit = 1u << ((i + j) & 31);
          if (!(nz >> j & 1)) wd &= ~bit;
          else if (wd & bit) ++out->header.label_counts[label_of(v >> (8 * j) & 255u)];
        }
      }
    for (size_t k = 0; k < bits.size(); ++k) { pre[k] = n; n += (uint32_t)__builtin_popcount(bits[k]); }
    out->header.n_cands = n;
    out->records.assign(n, Record{0, 0.0f});
    built = true;
  };
  auto emit = [&](int r, int c, uint32_t in_dword, uint32_t gone /* nibble */, float score) {
    const uint32_t i = (uint32_t)r * w + 4 * c, hit = gone & bits4(bits.data(), i);
    for (int j = 0; j < 4; ++j)
      if (hit >> j & 1) {
        const uint32_t k = i + j, slot = pre[k >> 5] + (uint32_t)__builtin_popcount(bits[k >> 5] & ((1u << (k & 31)) - 1u));
        out->records[slot] = Record{pack_xyl(4 * c + j, r, label_of(in_dword >> (8 * j) & 255u)), score};
      }
  };
  const int S = w > h ? w : h;
  const int thr1 = extract_threshold < 1 ? 1 : extract_threshold;
  std::vector<uint32_t>*in = &a, *o = &b;
  for (int s = 1; s <= S; ++s) {
    if (!built && s == thr1) build(*in);
    const uint32_t any = step_all(*in, *o, [&](int r, int c, uint32_t i, uint32_t ov) {
      if (built) emit(r, c, i, nonzero_nibble(i) & ~nonzero_nibble(ov) & (c == ws - 1 ? ~nonzero_nibble(pad) : 15u), (float)s);
    });
    std::vector<uint32_t>* t = in; in = o; o = t;
    if (!any) break;
  }
  if (!built) build(*in);
  for (int r = 0; r < h; ++r)
    for (int c = 0; c < ws; ++c) {
      const uint32_t v = (*in)[(size_t)r * ws + c];
      emit(r, c, v, nonzero_nibble(v) & (c == ws - 1 ? ~nonzero_nibble(pad) : 15u), (float)kNoZeroDistance);
    }
}
#endif  // LMX_TC_HOST

}  // namespace train_cand
}  // namespace lmx
