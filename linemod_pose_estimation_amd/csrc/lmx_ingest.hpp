// Ingest of frames that already live in device memory (lmx_ctx_upload_device, include/lmx.h): the node-side steps of lmx_ctx_upload_raw --
// MONO8 -> BGR, GaussianBlur 3x3 on the full frame ((sum + 8) >> 4, BORDER_REFLECT_101), crop, float metres -> u16 millimetres -- or a plain
// pitched copy, read straight from the caller's images through a table of {pointer, row stride} per frame and written into the frame set's
// level-0 buffers.  The body is shared by the HIP kernel (lmx_ingest.hip, k_ingest) and by plain CPU builds (LMX_INGEST_HOST, set for any
// compiler but hipcc: tests/cpp/ingest_host.cpp), where run() walks the kernel's grid with one "lane" at a time.
//
// Work item.  A modality's result row is `row_bytes` bytes BEFORE the MONO8 -> BGR expansion: W * source channels for colour, W * 2 for
// depth.  One lane takes one 16-byte chunk k of that row on kRows consecutive output rows (a strip); consecutive lanes take consecutive
// chunks, so a wave's accesses are contiguous on both sides.  With `expand3` every result byte is stored three times (48 bytes per chunk).
//
// Path selection, per frame (uniform in a workgroup: blockIdx.y is the frame):
//   wide    the source's base address and row stride are multiples of 16 and row_bytes is one (then every chunk is whole and every
//           destination chunk is 16-byte aligned: the frame buffers are, and a frame is H rows of row_bytes or 3 * row_bytes).  Every
//           global access is an aligned 16-byte load or store.  A chunk's window starts at source byte p = crop_x * px_bytes + 16 k
//           (- NB with the blur: NB = bytes per source pixel is the distance of a byte's horizontal neighbours), which is rarely a multiple
//           of 16: the lane loads the two or three aligned granules that hold the window and shifts them into place in registers (a
//           funnel shift by p & 3 on the dwords from p >> 2 & 3 on; both are the same in every lane of a launch, and the kernel
//           branches once on the latter to code with constant register indices).  Only granules that hold a byte of the source row
//           are addressed (clamped otherwise), so no load leaves a 16-byte granule that the image owns a byte of; the bytes a clamp
//           gets wrong lie outside the row, and exactly those are the ones BORDER_REFLECT_101 replaces (reflect_window).
//           Blur: the window's horizontal sums s[j - NB] + 2 s[j] + s[j + NB] are formed on packed 16-bit halves (even and odd bytes of
//           a dword), one row at a time; a strip keeps the sums of three source rows in registers and rolls them, so a source row is
//           loaded once per strip (kRows + 2 row loads for kRows output rows), not once per tap.
//           Float depth: a chunk is 8 results from 32 source bytes (two or three granules; the shift is whole dwords).
//   narrow  anything else (a base or stride that is only element-aligned, a width that gives no whole chunks): the same work item, element
//           by element with element-sized accesses, by the definitions (color_at, metres_to_mm).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if !defined(__HIPCC__) && !defined(LMX_INGEST_HOST)
#define LMX_INGEST_HOST   // a plain C++ compiler: the CPU build
#endif
#ifdef LMX_INGEST_HOST
#define LMX_IN_FN inline
#define LMX_IN_UNROLL
#else
#define LMX_IN_FN __host__ __device__ __forceinline__
#define LMX_IN_UNROLL _Pragma("unroll")   // the register arrays below are indexed by loop counters: full unrolling keeps them in registers
#endif

namespace lmx {
namespace ingest {

constexpr int kRows = 8;        // output rows per lane
constexpr int kBlock = 256;     // lanes per workgroup

enum Mode : int32_t {
  COPY = 0,      // result bytes = source bytes at the crop (BGR, MONO8, u16 depth; pre == NULL)
  BLUR1 = 1,     // 3x3 blur of a one-byte-per-pixel source (MONO8)
  BLUR3 = 2,     // 3x3 blur of a three-byte-per-pixel source (BGR)
  FLOAT_MM = 3,  // float metres -> u16 millimetres
};

struct Entry { uint64_t src; uint64_t row_stride; };   // one source image; the layout of PullEntry (lmx_internal.hpp)

struct Args {
  uint8_t* dst;             // frame 0 of the destination
  uint64_t dst_frame_bytes;
  int32_t SH, SW;           // source rows, pixels per source row
  int32_t H, W;             // output rows, pixels per output row
  int32_t crop_x, crop_y;
  int32_t px_bytes;         // bytes per source pixel: 1, 2 (u16), 3, 4 (float)
  int32_t expand3;          // every result byte three times (MONO8 -> BGR); COPY and BLUR1 only
  uint32_t row_bytes;       // result bytes per row before the expansion
};

struct U4 { uint32_t x, y, z, w; };

// 16-byte accesses at 16-byte aligned addresses; on the device through global-memory pointers (the images and the frames are device
// memory: global_load / global_store instead of the flat forms a pointer made from a table entry would get)
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t V4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) V4 GlobalV4;
#endif
LMX_IN_FN U4 load16(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const V4 t = *(const GlobalV4*)p;
  return U4{t.x, t.y, t.z, t.w};
#else
  U4 v;
  memcpy(&v, p, 16);
  return v;
#endif
}
LMX_IN_FN void store16(uint8_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
  V4 t;
  t.x = a; t.y = b; t.z = c; t.w = d;
  *(GlobalV4*)p = t;
#else
  const U4 v{a, b, c, d};
  memcpy(p, &v, 16);
#endif
}
// keeps the compiler from regrouping neighbouring 16-byte stores into another width (no instruction)
LMX_IN_FN void store_fence() { __asm__ __volatile__("" ::: "memory"); }
LMX_IN_FN float load_f32(const uint8_t* p) {   // p is 4-byte aligned
  float v;
  memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}
LMX_IN_FN void store_u16(uint8_t* p, uint32_t v) {   // p is 2-byte aligned
  const uint16_t t = (uint16_t)v;
  memcpy(__builtin_assume_aligned(p, 2), &t, 2);
}

LMX_IN_FN int reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
  return p;
}
// convertTo(CV_16UC1, 1000.0) on x86-64: v = z * 1000.f, round half to even, saturate; NaN, Inf and |v| >= 2^31 give 0
LMX_IN_FN uint32_t metres_to_mm(float z) {
  const float v = z * 1000.f;
  if (!(v > -2147483648.f && v < 2147483648.f)) return 0u;
  const float r = rintf(v);
  return r < 0.f ? 0u : (r > 65535.f ? 65535u : (uint32_t)r);
}
// one byte of the colour result by the definition: source byte j of output row y (j counts the row's result bytes)
LMX_IN_FN uint32_t color_at(const Args& a, const uint8_t* src, size_t stride, int y, int j, bool blur) {
  const int sc = a.px_bytes, x = j / sc, ch = j - x * sc;
  const int sy = a.crop_y + y, sx = a.crop_x + x;
  if (!blur) return src[(size_t)sy * stride + (size_t)sx * sc + ch];
  int acc = 0;
  for (int dy = -1; dy <= 1; ++dy) {
    const uint8_t* row = src + (size_t)reflect101(sy + dy, a.SH) * stride;
    const int r = row[reflect101(sx - 1, a.SW) * sc + ch] + 2 * row[sx * sc + ch] + row[reflect101(sx + 1, a.SW) * sc + ch];
    acc += dy == 0 ? 2 * r : r;
  }
  return (uint32_t)((acc + 8) >> 4);
}

// ---- register work of the wide path --------------------------------------------------------------------------------------------------
// bytes [sb, sb + 4) of the 8 bytes lo | hi << 32, sb in 0 .. 3
LMX_IN_FN uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sb) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sb)); }
LMX_IN_FN uint32_t byte_at(const uint32_t* w, int i) { return w[i >> 2] >> (8 * (i & 3)) & 255u; }
LMX_IN_FN void put_byte(uint32_t* w, int i, uint32_t v) { w[i >> 2] = (w[i >> 2] & ~(255u << (8 * (i & 3)))) | v << (8 * (i & 3)); }

// The N dwords that start 4 SD + sb bytes into the granules g[0 .. 12); N <= 8.  The dword part of the shift is a template parameter (wide_item
// is instantiated for its four values and chosen by a uniform branch), so that every register index is a constant.
template <int N, int SD>
LMX_IN_FN void shift_window(const uint32_t (&g)[12], uint32_t sb, uint32_t (&out)[N]) {
  static_assert(N <= 8 && SD >= 0 && SD <= 3, "g[N + SD] must exist");
LMX_IN_UNROLL
  for (int i = 0; i < N; ++i) out[i] = funnel(g[i + SD], g[i + SD + 1], sb);
}

// Granules G, G + 1 (and G + 2 when `three`) of a source row whose last granule with a byte of the row is `last`; G may be -1.
LMX_IN_FN void load_granules(const uint8_t* row, int G, int last, bool two, bool three, uint32_t (&g)[12]) {
  const int g0 = G < 0 ? 0 : G, g1 = G + 1 > last ? last : G + 1, g2 = G + 2 > last ? last : G + 2;
  const U4 a = load16(row + (size_t)g0 * 16);
  g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w;
  g[4] = g[5] = g[6] = g[7] = g[8] = g[9] = g[10] = g[11] = 0u;
  if (two) {
    const U4 b = load16(row + (size_t)g1 * 16);
    g[4] = b.x; g[5] = b.y; g[6] = b.z; g[7] = b.w;
  }
  if (three) {
    const U4 c = load16(row + (size_t)g2 * 16);
    g[8] = c.x; g[9] = c.y; g[10] = c.z; g[11] = c.w;
  }
}

// BORDER_REFLECT_101 on a blur window w = source bytes [p, p + 16 + 2 NB): pixel -1 is pixel 1, pixel SW is pixel SW - 2.  A window leaves
// the row only by one pixel, on the left iff p == -NB, on the right iff it ends NB bytes behind the row.
template <int NB>
LMX_IN_FN void reflect_window(uint32_t* w, bool left, bool right) {
  if (left) {
LMX_IN_UNROLL
    for (int i = 0; i < NB; ++i) put_byte(w, i, byte_at(w, 2 * NB + i));
  }
  if (right) {
LMX_IN_UNROLL
    for (int i = 0; i < NB; ++i) put_byte(w, 16 + NB + i, byte_at(w, 16 - NB + i));
  }
}

struct HSum { uint32_t e[4], o[4]; };   // horizontal sums of 16 bytes as 16-bit halves: e = bytes 0, 2 of each dword, o = bytes 1, 3

// s[j - NB] + 2 s[j] + s[j + NB] for the 16 bytes j of chunk k of source row `ry`
template <int NB, int SD>
LMX_IN_FN HSum blur_row(const Args& a, const uint8_t* src, size_t stride, int ry, uint32_t k) {
  const int src_row_bytes = a.SW * NB;
  const int p = a.crop_x * NB + (int)(16u * k) - NB;       // >= -NB
  const int G = p < 0 ? -1 : p >> 4, last = (src_row_bytes - 1) >> 4;
  const uint32_t s = (uint32_t)(p + 16) & 15u;
  uint32_t g[12], w[6];
  load_granules(src + (size_t)ry * stride, G, last, true, s + 16 + 2 * NB > 32, g);
  shift_window<6, SD>(g, s & 3u, w);
  reflect_window<NB>(w, p < 0, p + 16 + 2 * NB > src_row_bytes);
  HSum h;
LMX_IN_UNROLL
  for (int i = 0; i < 4; ++i) {
    const uint32_t A = w[i];
    const uint32_t B = NB == 1 ? funnel(w[i], w[i + 1], 1) : funnel(w[i], w[i + 1], 3);
    const uint32_t C = NB == 1 ? funnel(w[i], w[i + 1], 2) : funnel(w[i + 1], w[i + 2], 2);
    h.e[i] = (A & 0x00ff00ffu) + 2u * (B & 0x00ff00ffu) + (C & 0x00ff00ffu);
    h.o[i] = (A >> 8 & 0x00ff00ffu) + 2u * (B >> 8 & 0x00ff00ffu) + (C >> 8 & 0x00ff00ffu);
  }
  return h;
}

// 16 result bytes r[0 .. 4) of output row y, chunk k: as they are, or every byte three times
LMX_IN_FN void store_chunk(const Args& a, uint8_t* dst, int y, uint32_t k, const uint32_t* r) {
  if (!a.expand3) {
    store16(dst + (size_t)y * a.row_bytes + 16u * k, r[0], r[1], r[2], r[3]);
    return;
  }
  uint32_t o[12];
LMX_IN_UNROLL
  for (int d = 0; d < 12; ++d)
    o[d] = byte_at(r, (4 * d) / 3) | byte_at(r, (4 * d + 1) / 3) << 8 | byte_at(r, (4 * d + 2) / 3) << 16 | byte_at(r, (4 * d + 3) / 3) << 24;
  uint8_t* p = dst + (size_t)y * a.row_bytes * 3 + 48u * k;
  store16(p, o[0], o[1], o[2], o[3]);
  store_fence();
  store16(p + 16, o[4], o[5], o[6], o[7]);
  store_fence();
  store16(p + 32, o[8], o[9], o[10], o[11]);
}

// the first source byte of chunk 0's window, + 16 (never negative); its low four bits are every chunk's shift
LMX_IN_FN uint32_t window_start(const Args& a, int mode) {
  return (uint32_t)(a.crop_x * a.px_bytes + 16 - (mode == BLUR1 ? 1 : (mode == BLUR3 ? 3 : 0)));
}

template <int MODE, int SD>
LMX_IN_FN void wide_item(const Args& a, const uint8_t* src, size_t stride, uint8_t* dst, int y0, int y1, uint32_t k) {
  if (MODE == COPY) {
    const uint32_t p = (uint32_t)a.crop_x * (uint32_t)a.px_bytes + 16u * k, s = p & 15u;
    for (int y = y0; y < y1; ++y) {
      uint32_t g[12], r[4];
      // the chunk's 16 bytes lie inside the row: granule G + 1 holds one of them whenever s != 0
      load_granules(src + (size_t)(a.crop_y + y) * stride, (int)(p >> 4), (int)((p + 15u) >> 4), s != 0, false, g);
      shift_window<4, SD>(g, s & 3u, r);
      store_chunk(a, dst, y, k, r);
    }
  } else if (MODE == FLOAT_MM) {
    const uint32_t p = (uint32_t)a.crop_x * 4u + 32u * k, s = p & 15u;   // a multiple of 4
    for (int y = y0; y < y1; ++y) {
      uint32_t g[12], w[8], r[4];
      load_granules(src + (size_t)(a.crop_y + y) * stride, (int)(p >> 4), (int)((p + 31u) >> 4), true, s != 0, g);
      shift_window<8, SD>(g, s & 3u, w);
LMX_IN_UNROLL
      for (int i = 0; i < 4; ++i) {
        float lo, hi;
        memcpy(&lo, &w[2 * i], 4);
        memcpy(&hi, &w[2 * i + 1], 4);
        r[i] = metres_to_mm(lo) | metres_to_mm(hi) << 16;
      }
      store_chunk(a, dst, y, k, r);
    }
  } else {
    constexpr int NB = MODE == BLUR1 ? 1 : 3;
    HSum up = blur_row<NB, SD>(a, src, stride, reflect101(a.crop_y + y0 - 1, a.SH), k);
    HSum mid = blur_row<NB, SD>(a, src, stride, a.crop_y + y0, k);
    for (int y = y0; y < y1; ++y) {
      const HSum dn = blur_row<NB, SD>(a, src, stride, reflect101(a.crop_y + y + 1, a.SH), k);
      uint32_t r[4];
LMX_IN_UNROLL
      for (int i = 0; i < 4; ++i) {
        const uint32_t e = (up.e[i] + 2u * mid.e[i] + dn.e[i] + 0x00080008u) >> 4 & 0x00ff00ffu;
        const uint32_t o = (up.o[i] + 2u * mid.o[i] + dn.o[i] + 0x00080008u) >> 4 & 0x00ff00ffu;
        r[i] = e | o << 8;
      }
      store_chunk(a, dst, y, k, r);
      up = mid;
      mid = dn;
    }
  }
}

template <int MODE>
LMX_IN_FN void narrow_item(const Args& a, const uint8_t* src, size_t stride, uint8_t* dst, int y0, int y1, uint32_t k) {
  const uint32_t j0 = 16u * k, j1 = j0 + 16u < a.row_bytes ? j0 + 16u : a.row_bytes;
  for (int y = y0; y < y1; ++y) {
    if (MODE == FLOAT_MM) {
      const uint8_t* row = src + (size_t)(a.crop_y + y) * stride + (size_t)a.crop_x * 4;
      for (uint32_t j = j0; j < j1; j += 2) store_u16(dst + (size_t)y * a.row_bytes + j, metres_to_mm(load_f32(row + 2 * (size_t)j)));
    } else {
      for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t v = color_at(a, src, stride, y, (int)j, MODE != COPY);
        if (a.expand3) {
          uint8_t* p = dst + ((size_t)y * a.row_bytes + j) * 3;
          p[0] = p[1] = p[2] = (uint8_t)v;
        } else {
          dst[(size_t)y * a.row_bytes + j] = (uint8_t)v;
        }
      }
    }
  }
}

LMX_IN_FN uint32_t chunks_per_row(const Args& a) { return (a.row_bytes + 15u) >> 4; }
LMX_IN_FN uint32_t strips(const Args& a) { return ((uint32_t)a.H + kRows - 1) / kRows; }
LMX_IN_FN uint32_t items_per_frame(const Args& a) { return chunks_per_row(a) * strips(a); }
LMX_IN_FN bool is_wide(const Args& a, const Entry& e) { return ((e.src | e.row_stride | (uint64_t)a.row_bytes) & 15u) == 0; }

// work item `item` (< items_per_frame) of frame `frame`
template <int MODE>
LMX_IN_FN void run_item(const Args& a, const Entry& e, uint32_t frame, uint32_t item) {
  const uint32_t n = chunks_per_row(a), strip = item / n, k = item - strip * n;
  const int y0 = (int)strip * kRows, y1 = y0 + kRows < a.H ? y0 + kRows : a.H;
  const uint8_t* src = reinterpret_cast<const uint8_t*>((uintptr_t)e.src);
  uint8_t* dst = a.dst + (size_t)frame * a.dst_frame_bytes;
  if (is_wide(a, e)) {
    switch (window_start(a, MODE) >> 2 & 3u) {   // the same in every lane of the launch
      case 0: wide_item<MODE, 0>(a, src, (size_t)e.row_stride, dst, y0, y1, k); break;
      case 1: wide_item<MODE, 1>(a, src, (size_t)e.row_stride, dst, y0, y1, k); break;
      case 2: wide_item<MODE, 2>(a, src, (size_t)e.row_stride, dst, y0, y1, k); break;
      default: wide_item<MODE, 3>(a, src, (size_t)e.row_stride, dst, y0, y1, k); break;
    }
  }
  else narrow_item<MODE>(a, src, (size_t)e.row_stride, dst, y0, y1, k);
}

// The launch of one modality (everything of Args but dst) -> its Mode.  Colour: src_channels 1 | 3 into dst_channels 1 | 3 (3 -> 1 does not
// exist); depth: u16, or float metres.  The source is SW x SH, the output the W x H at (crop_x, crop_y) of it (blur: of the blurred source).
inline int plan(Args* a, bool color, int src_channels, int dst_channels, bool blur, bool depth_float, int SH, int SW, int H, int W, int crop_x, int crop_y) {
  a->SH = SH; a->SW = SW; a->H = H; a->W = W; a->crop_x = crop_x; a->crop_y = crop_y;
  a->px_bytes = color ? src_channels : (depth_float ? 4 : 2);
  a->expand3 = color && src_channels == 1 && dst_channels == 3 ? 1 : 0;
  a->row_bytes = (uint32_t)W * (uint32_t)(color ? src_channels : 2);
  a->dst_frame_bytes = (uint64_t)H * a->row_bytes * (a->expand3 ? 3u : 1u);
  if (!color) return depth_float ? FLOAT_MM : COPY;
  return !blur ? COPY : (src_channels == 1 ? BLUR1 : BLUR3);
}

#ifdef LMX_INGEST_HOST
// ---- the kernel's whole grid on the CPU, one lane at a time: what tests/cpp/ingest_host.cpp runs ---------------------------------------
inline void run(int mode, const Args& a, const Entry* tab, int n_frames) {
  for (int f = 0; f < n_frames; ++f)
    for (uint32_t item = 0; item < items_per_frame(a); ++item) {
      if (mode == COPY) run_item<COPY>(a, tab[f], (uint32_t)f, item);
      else if (mode == BLUR1) run_item<BLUR1>(a, tab[f], (uint32_t)f, item);
      else if (mode == BLUR3) run_item<BLUR3>(a, tab[f], (uint32_t)f, item);
      else run_item<FLOAT_MM>(a, tab[f], (uint32_t)f, item);
    }
}
#endif

}  // namespace ingest
}  // namespace lmx
