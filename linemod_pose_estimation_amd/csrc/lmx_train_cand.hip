// Candidate lists of the mesh trainer on the device (lmx_bank_train_mesh_opts, LMX_TRAIN_CANDIDATES_DEVICE): the per-pixel half of
// extractTemplate, so that only the lists cross PCIe instead of every window's magnitudes, labels and mask.  The definitions, the window
// image and the list format are lmx_train_cand.hpp; this file is the parallel shape:
//
//   k_train_candidates  one workgroup of 256 lanes per (view, pyramid level, modality), the window (mesh_window of the state words, what
//                       k_mesh_pack copies) in LDS.
//                       ColorGradient: the mask's inner contour by a 3x3 minimum on the LDS copy, q and mag read only there; wave ballots
//                       give a bitmap of the candidates, a prefix over its words their places, one atomicAdd on the batch's bump counter
//                       the list's place, and a second walk writes the records.
//                       DepthNormal: two AND steps erode the mask, temp = local ? q : 0 becomes the window image, and the AND steps run
//                       (ping-pong between two LDS images, one barrier each) until the image is all zero or max(w, h) steps are done.  A
//                       pixel is a candidate iff its one-hot bit survives extract_threshold - 1 steps: at that step the bitmap, the
//                       label counts, the prefix and the list's place are fixed, and from then on the step that clears a candidate's
//                       bit writes its record -- {x, y, label, step} -- straight to its place, so no per-pixel distance is stored.
//                       Bits that survive every step get (float)(1 << 28).
//   k_train_cand_copy   copies the batch's records [0, bump) from device memory to the pinned host buffer with 16-byte stores (the records
//                       are written in scattered 8-byte stores, which device memory takes well and PCIe does not).
// A list's place in the buffer depends on the order in which the workgroups reserve; its contents do not.  No workgroup waits for another.
#include "lmx_internal.hpp"
#include "lmx_train_cand.hpp"

namespace lmx {
namespace {

namespace tc = train_cand;

struct CandShared {
  uint32_t img[2][tc::kMaxWindowDwords];
  uint32_t bits[tc::kMaxBitWords + 2], pre[tc::kMaxBitWords + 2];
  uint32_t scan[256];
  uint32_t counts[8];
  uint32_t area, total, offset, ok;
};

// pre[k] = number of set bits in bits[0 .. k); sh.total = all of them.  Every lane calls it.
__device__ void bitmap_prefix(CandShared& sh, int n_words) {
  const int tid = threadIdx.x, per = (n_words + 255) / 256;
  const int k0 = min(tid * per, n_words), k1 = min(k0 + per, n_words);
  uint32_t sum = 0;
  for (int k = k0; k < k1; ++k) sum += __popc(sh.bits[k]);
  sh.scan[tid] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint32_t add = tid >= d ? sh.scan[tid - d] : 0u;
    __syncthreads();
    sh.scan[tid] += add;
    __syncthreads();
  }
  uint32_t run = tid > 0 ? sh.scan[tid - 1] : 0u;
  for (int k = k0; k < k1; ++k) { sh.pre[k] = run; run += __popc(sh.bits[k]); }
  if (tid == 255) sh.total = sh.scan[255];
  __syncthreads();
}

// One lane reserves the list's place; -> false when it does not fit (nothing may be written then).
__device__ bool reserve_list(CandShared& sh, const TrainCandArgs& a) {
  if (threadIdx.x == 0) {
    const uint32_t off = atomicAdd(a.bump, sh.total);
    sh.offset = off;
    sh.ok = (uint64_t)off + sh.total <= (uint64_t)a.cap;
  }
  __syncthreads();
  return sh.ok != 0;
}

__device__ void write_header(const CandShared& sh, tc::ListHeader* hd, uint32_t n, uint32_t status) {
  if (threadIdx.x == 0) {
    hd->n_cands = n; hd->area = sh.area; hd->status = status; hd->offset = sh.offset;
    for (int k = 0; k < 8; ++k) hd->label_counts[k] = sh.counts[k];
    for (int k = 0; k < 4; ++k) hd->reserved[k] = 0;
  }
}

__device__ uint32_t slot_of(const CandShared& sh, uint32_t i) { return sh.pre[i >> 5] + __popc(sh.bits[i >> 5] & ((1u << (i & 31)) - 1u)); }

__global__ __launch_bounds__(256) void k_train_candidates(TrainCandArgs a) {
  __shared__ CandShared sh;
  const int m = blockIdx.x, l = blockIdx.y, v = blockIdx.z, tid = threadIdx.x;
  const int32_t* st = a.state + (size_t)v * kMeshStateWords;
  if (st[MS_INVALID]) return;   // the call fails: nothing of this view is used
  tc::ListHeader* hd = a.headers + ((size_t)v * a.n_levels + l) * a.n_mod + m;
  const int wl = a.W >> l, hl = a.H >> l;
  int wx0, wy0, w, h;
  mesh_window(st + MS_LEVEL + 4 * l, wl, hl, &wx0, &wy0, &w, &h);
  if (tid < 8) sh.counts[tid] = 0;
  if (tid == 0) { sh.area = 0; sh.total = 0; sh.offset = 0; sh.ok = 0; }
  __syncthreads();
  if (!tc::window_fits(w, h)) { write_header(sh, hd, 0, tc::ST_TOO_LARGE); return; }
  const int ws = tc::row_dwords(w), n_dwords = ws * h, n_px = w * h, n_words = (n_px + 31) >> 5;
  const uint32_t pad = tc::pad_mask(w);
  const size_t px0 = (size_t)a.W * a.H, fpx = (size_t)wl * hl;
  // level 0's images at (y << l, x << l): the mask, and DepthNormal's labels (upstream's nearest-neighbour chain)
  const uint8_t* mask0 = a.mask0 ? a.mask0 + (size_t)v * px0 : nullptr;
  auto at0 = [&](int r, int x) -> size_t { return (size_t)((wy0 + r) << l) * a.W + ((wx0 + x) << l); };
  for (int k = tid; k < n_words + 2; k += 256) sh.bits[k] = 0;
  __syncthreads();

  if (a.mag[l][m]) {
    // ---- ColorGradient ----------------------------------------------------------------------------------------------------------------
    uint8_t* mk = reinterpret_cast<uint8_t*>(sh.img[0]);   // raw mask bytes, rows of 4 * ws
    if (mask0)
      for (int i = tid; i < n_px; i += 256) { const int r = i / w, x = i - r * w; mk[r * 4 * ws + x] = mask0[at0(r, x)]; }
    __syncthreads();
    const uint8_t* q = a.quant[l][m] + (size_t)v * fpx;
    const float* mg = a.mag[l][m] + (size_t)v * fpx;
    const float thr = tc::color_threshold_sq(a.strong_threshold[m]);
    auto is_cand = [&](int i) -> bool {
      const int r = i / w, x = i - r * w;
      uint32_t mc = 0, mn = 255;
      if (mask0) {
        mc = mk[r * 4 * ws + x];
        for (int dy = -1; dy <= 1; ++dy) {
          const uint8_t* row = mk + tc::clampi(r + dy, 0, h - 1) * 4 * ws;
          for (int dx = -1; dx <= 1; ++dx) mn = min(mn, (uint32_t)row[tc::clampi(x + dx, 0, w - 1)]);
        }
        if (!(mc > mn)) return false;   // q and mag are read on the contour only
      }
      const size_t o = (size_t)(wy0 + r) * wl + (wx0 + x);
      return tc::color_candidate(mask0 != nullptr, mc, mn, q[o], mg[o], thr);
    };
    for (int base = 0; base < n_px; base += 256) {   // a wave covers 64 consecutive pixels = two bitmap words
      const int i = base + tid;
      const unsigned long long bal = __ballot(i < n_px && is_cand(i));
      if ((tid & 63) == 0 && i < n_px) { sh.bits[i >> 5] = (uint32_t)bal; sh.bits[(i >> 5) + 1] = (uint32_t)(bal >> 32); }
    }
    __syncthreads();
    bitmap_prefix(sh, n_words);
    const uint32_t n = sh.total;
    if (!reserve_list(sh, a)) { write_header(sh, hd, n, tc::ST_OVERFLOW); return; }
    tc::Record* out = a.records + sh.offset;
    for (int i = tid; i < n_px; i += 256)
      if (sh.bits[i >> 5] >> (i & 31) & 1u) {
        const int r = i / w, x = i - r * w;
        const size_t o = (size_t)(wy0 + r) * wl + (wx0 + x);
        out[slot_of(sh, (uint32_t)i)] = tc::Record{tc::pack_xyl(x, r, tc::label_of(q[o])), mg[o]};
      }
    write_header(sh, hd, n, 0);
    return;
  }

  // ---- DepthNormal ----------------------------------------------------------------------------------------------------------------------
  const uint8_t* q0 = a.quant[0][m] + (size_t)v * px0;
  int thr = a.extract_threshold[m];
  for (int k = 0; k < l; ++k) thr /= 2;
  auto load4 = [&](const uint8_t* src, int r, int c, bool as_mask) -> uint32_t {
    uint32_t val = 0;
    for (int j = 0; j < 4; ++j) {
      const int x = 4 * c + j;
      if (x < w) { const uint32_t b = src[at0(r, x)]; val |= (as_mask ? (b ? 255u : 0u) : b) << (8 * j); }
    }
    return val;
  };
  const int n_chunks = (h + tc::kStepRows - 1) / tc::kStepRows, n_items = n_chunks * ws;
  // every lane runs one AND step over its work items (dword column c, kStepRows rows), in -> out
  auto step = [&](const uint32_t* in, uint32_t* out, auto&& on_dword) -> uint32_t {
    uint32_t any = 0;
    for (int it = tid; it < n_items; it += 256) {
      const int ch = it / ws, c = it - ch * ws, r0 = ch * tc::kStepRows;
      any |= tc::and_step_rows(in, out, ws, h, pad, c, r0, min(r0 + tc::kStepRows, h), [&](int r, uint32_t i, uint32_t o) { on_dword(r, c, i, o); });
    }
    return any;
  };
  auto nothing = [](int, int, uint32_t, uint32_t) {};
  if (mask0) {   // local: mask != 0 eroded twice
    for (int d = tid; d < n_dwords; d += 256) { const int r = d / ws, c = d - r * ws; sh.img[0][d] = load4(mask0, r, c, true) | (c == ws - 1 ? pad : 0u); }
    __syncthreads();
    step(sh.img[0], sh.img[1], nothing);
    __syncthreads();
    step(sh.img[1], sh.img[0], nothing);
    __syncthreads();
  }
  uint32_t area = 0;
  for (int d = tid; d < n_dwords; d += 256) {
    const int r = d / ws, c = d - r * ws;
    const uint32_t pm = c == ws - 1 ? pad : 0u;
    const uint32_t loc = mask0 ? sh.img[0][d] & ~pm : ~pm;
    const uint32_t t = load4(q0, r, c, false) & loc;
    area += (uint32_t)__popc(loc) >> 3;
    sh.img[0][d] = t | pm;
    const uint32_t oh = tc::onehot_nibble(t), i = (uint32_t)(r * w + 4 * c), shf = i & 31;
    if (oh) {
      atomicOr(&sh.bits[i >> 5], oh << shf);
      if (shf > 28) atomicOr(&sh.bits[(i >> 5) + 1], oh >> (32 - shf));
    }
  }
  if (area) atomicAdd(&sh.area, area);
  __syncthreads();

  const bool thr_reachable = (int64_t)thr <= (int64_t)tc::kNoZeroDistance;
  // fixes the candidates from the image after max(thr, 1) - 1 steps: one-hot pixels whose byte is still non-zero.  -> list fits
  auto build = [&](const uint32_t* in) -> bool {
    uint32_t lo = 0, hi = 0;   // label counts of this lane, 8 bits each (a lane sees <= 64 dwords = 256 pixels: flushed every 16 dwords)
    int seen = 0;
    auto flush = [&]() {
      for (int k = 0; k < 4; ++k) {
        if (lo >> (8 * k) & 255u) atomicAdd(&sh.counts[k], lo >> (8 * k) & 255u);
        if (hi >> (8 * k) & 255u) atomicAdd(&sh.counts[4 + k], hi >> (8 * k) & 255u);
      }
      lo = hi = 0;
    };
    for (int d = tid; d < n_dwords; d += 256) {
      const int r = d / ws, c = d - r * ws;
      const uint32_t val = in[d], i = (uint32_t)(r * w + 4 * c), shf = i & 31;
      const uint32_t valid = c == ws - 1 ? ~tc::nonzero_nibble(pad) & 15u : 15u;
      const uint32_t nz = thr_reachable ? tc::nonzero_nibble(val) : 0u;
      const uint32_t old = tc::bits4(sh.bits, i) & valid, clr = old & ~nz, keep = old & nz;
      if (clr) {
        atomicAnd(&sh.bits[i >> 5], ~(clr << shf));
        if (shf > 28) atomicAnd(&sh.bits[(i >> 5) + 1], ~(clr >> (32 - shf)));
      }
      for (int j = 0; j < 4; ++j)
        if (keep >> j & 1u) {
          const int lab = __ffs((int)(val >> (8 * j) & 255u)) - 1;
          if (lab < 4) lo += 1u << (8 * lab); else hi += 1u << (8 * (lab - 4));
        }
      if (++seen == 16) { flush(); seen = 0; }
    }
    flush();
    __syncthreads();
    bitmap_prefix(sh, n_words);
    return reserve_list(sh, a);
  };
  // NOTE on build()'s bits4 / atomicAnd: a lane only clears bits of its own pixels, and bits4 reads only decide about those.
  auto emit = [&](int r, int c, uint32_t in_dword, uint32_t gone, float score) {
    const uint32_t i = (uint32_t)(r * w + 4 * c), hit = gone & tc::bits4(sh.bits, i);
    for (int j = 0; j < 4; ++j)
      if (hit >> j & 1u) a.records[sh.offset + slot_of(sh, i + j)] = tc::Record{tc::pack_xyl(4 * c + j, r, tc::label_of(in_dword >> (8 * j) & 255u)), score};
  };
  const uint32_t valid_last = ~tc::nonzero_nibble(pad) & 15u;
  const int S = max(w, h), thr1 = max(thr, 1);
  bool built = false, fits = true;
  int cur = 0;
  for (int s = 1; s <= S; ++s) {
    if (!built && s == thr1) { fits = build(sh.img[cur]); built = true; if (!fits) break; }
    const float score = (float)s;
    const uint32_t any = step(sh.img[cur], sh.img[cur ^ 1], [&](int r, int c, uint32_t i, uint32_t o) {
      if (built) emit(r, c, i, tc::nonzero_nibble(i) & ~tc::nonzero_nibble(o) & (c == ws - 1 ? valid_last : 15u), score);
    });
    cur ^= 1;
    if (!__syncthreads_or(any != 0)) break;
  }
  if (!built) fits = build(sh.img[cur]);
  if (!fits) { write_header(sh, hd, sh.total, tc::ST_OVERFLOW); return; }
  for (int d = tid; d < n_dwords; d += 256) {   // bits that no step cleared
    const int r = d / ws, c = d - r * ws;
    const uint32_t val = sh.img[cur][d];
    emit(r, c, val, tc::nonzero_nibble(val) & (c == ws - 1 ? valid_last : 15u), (float)tc::kNoZeroDistance);
  }
  write_header(sh, hd, sh.total, 0);
}

__global__ __launch_bounds__(256) void k_train_cand_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, const uint32_t* __restrict__ bump, uint32_t cap) {
  const uint32_t n = min(*bump, cap);          // records; an overflowing list reserved without writing
  const size_t n16 = ((size_t)n + 1) / 2;      // the buffers hold an even number of records
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

}  // namespace

void launch_train_candidates(hipStream_t s, const TrainCandArgs& a, int n_views) {
  hipLaunchKernelGGL(k_train_candidates, dim3((unsigned)a.n_mod, (unsigned)a.n_levels, (unsigned)n_views), dim3(256), 0, s, a);
}

void launch_train_cand_copy(hipStream_t s, const TrainCandArgs& a, train_cand::Record* host_dst) {
  hipLaunchKernelGGL(k_train_cand_copy, dim3(256), dim3(256), 0, s, reinterpret_cast<const uint4*>(a.records), reinterpret_cast<uint4*>(host_dst), a.bump, a.cap);
}

}  // namespace lmx
