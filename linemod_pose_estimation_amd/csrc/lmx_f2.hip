// SURVEY.md 8f row 2 on the device: the immediate consumer of match() --
//   Detector::match's own std::sort + std::unique (upstream A.10), then the reference's
//   rcd_voting -> cluster_filter -> cluster_scoring -> nonMaximaSuppressionUsingIOU
//   (/root/reference/src/rgbdDetector.cpp:36-70, 72-85, 118-144, 462-574; chained at
//   src/linemod_ensenso_detect_3_mult_detect_service.cpp:376-447)
// -- as ONE kernel that consumes the raw-match slot written by k_refine, one workgroup per frame, everything in LDS.
//
// Both std::sort calls of that chain are unstable sorts whose order of ties is observable (std::unique removes ADJACENT duplicates;
// the greedy NMS walks the clusters in sorted order), so the kernel reproduces libstdc++'s algorithm: the big sort (stage C, up to 2048
// records) with lmx_sort_block.hpp, the workgroup-parallel form that yields the same permutation (round 3: the one-lane emulation took
// 1.4 ms at 500 records per frame, twice the host path; profiles/r03_f2_timing.txt), the small one (stage G, a handful of clusters) with
// the sequential restatement lmx_sort_emul.hpp on one lane:
//   A  collect the frame's records from the slot (all frames of a batch share one list)            parallel, LDS append
//   B  restore upstream insertion order: bitonic sort by order_key (keys are unique)                parallel
//   C  std::sort by Match::operator< (similarity desc, template_id asc)                             parallel emulated introsort
//   D  std::unique (x, y, similarity, class equal; == is an equivalence, so "equal to the previous" decides)   parallel + block scan
//   E  rcd_voting: key = {y / step, x / step, depth ring}; std::map order = bitonic sort by (key, position in the match list)
//   F  clusters = runs of equal key: size filter, mean similarity (double), mean rect (integer division)       lane 0
//   G  std::sort by score desc (emulated) + greedy IoU suppression at 0.4 with the reference's int/float arithmetic   lane 0
// Frames with more than F2_MAX records are flagged (status 1); up to F2_LARGE_MAX records the large-frame form at the end of this file
// finishes them in a second launch, beyond that the host path (lmx_cluster_matches), so the result is the reference's for every input.
// The SCORED instantiation (lmx_ctx_collect_clusters_depth) ranks clusters by the reference's other score, the depth difference of
// depth_normal_diff_calc: every raw record comes with a lmx_depth_diff_t (k_depth_diff_records, lmx_verify.hip) that travels with it through
// B - D in two rows of device memory (LDS is full) and lands next to its final match; F averages dv::value of it instead of the similarity.
// The NORMAL instantiation (lmx_ctx_collect_clusters_depth_normal) carries a lmx_normal_diff_t (k_verify_diff_records) the same way in two
// rows of its own -- the 64 KB of LDS the sorts need at 2048 records leave no room for a second 16-byte payload, and an index into the
// per-record arrays would make lane 0's loop in F chase it through the unsorted list -- and averages nv::value of the pair.
#include <hip/hip_runtime.h>

#include "lmx_internal.hpp"
#include "lmx_depth_verify.hpp"
#include "lmx_normal_verify.hpp"
#include "lmx_sort_block.hpp"
#include "lmx_sort_emul.hpp"

namespace lmx {

namespace {

__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* key, int n_pow2, int tid, int nthreads) {
  for (int k = 2; k <= n_pow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n_pow2; i += nthreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = key[i], b = key[ixj];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { key[i] = b; key[ixj] = a; }
        }
      }
      __syncthreads();
    }
}

// the reference's computeIoU (rgbdDetector.cpp:532-574): boxes as {x, y, w, h}; int products converted to float, float division
// (wrapping int arithmetic spelled out, as in lmx_cluster.cpp's box_overlap_ratio: rects of clusters left of / above the origin are huge)
__device__ __forceinline__ int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int wsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int wmul(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
__device__ float box_iou(const int* p, const int* q) {
  const int p_x0 = p[0], p_x1 = wsub(wadd(p[0], p[2]), 1), p_y0 = p[1], p_y1 = wsub(wadd(p[1], p[3]), 1);
  const int q_x0 = q[0], q_x1 = wsub(wadd(q[0], q[2]), 1), q_y0 = q[1], q_y1 = wsub(wadd(q[1], q[3]), 1);
  const int lo_x = max(p_x0, q_x0), hi_x = min(p_x1, q_x1), lo_y = max(p_y0, q_y0), hi_y = min(p_y1, q_y1);
  const bool overlap_x = (lo_x >= p_x0 && lo_x <= p_x1) || (lo_x >= q_x0 && lo_x <= q_x1);
  const bool overlap_y = (lo_y >= p_y0 && lo_y <= p_y1) || (lo_y >= q_y0 && lo_y <= q_y1);
  const float shared = (overlap_x && overlap_y) ? (float)wmul(wadd(wsub(hi_x, lo_x), 1), wadd(wsub(hi_y, lo_y), 1)) : 0.0f;
  const float total = (float)wadd(wmul(p[2], p[3]), wmul(q[2], q[3])) - shared;
  return shared / total;
}

}  // namespace

// `int v; v /= n;` with n a size_t, as the reference writes it: v is converted to size_t first (value mod 2^64), the quotient back to int
__device__ __forceinline__ int div_by_size(int v, int n) {
  return (int)(unsigned)((unsigned long long)(long long)v / (unsigned long long)n);
}

// Match::operator< as one unsigned comparison: similarity descending (IEEE bits made order-preserving, then inverted), template_id
// ascending (signed -> offset binary).  Equal keys <=> neither element is less than the other.
__device__ __forceinline__ unsigned long long match_sort_key(float similarity, int template_id) {
  uint32_t b = __float_as_uint(similarity);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)(~b) << 32) | (unsigned long long)((uint32_t)template_id ^ 0x80000000u);
}

// test hook (lmx_debug_device_sort_perm): the permutation sortblk::sort produces for n <= F2_MAX (similarity, template_id) pairs
__global__ __launch_bounds__(256) void k_debug_block_sort(const float* sim, const int* tid_in, int n, int* perm, unsigned long long* spill) {
  __shared__ unsigned long long s_key[F2_MAX];
  __shared__ unsigned short s_tag[F2_MAX], s_seg[F2_MAX], s_lpos[F2_MAX], s_rpos[F2_MAX];
  __shared__ uint32_t s_cut[F2_MAX / 32];
  __shared__ sortblk::Scratch S;
  if (threadIdx.x == 0) { S.seg = s_seg; S.lpos = s_lpos; S.rpos = s_rpos; S.cut_bits = s_cut; }
  for (int i = threadIdx.x; i < n; i += 256) { s_key[i] = match_sort_key(sim[i], tid_in[i]); s_tag[i] = (unsigned short)i; }
  __syncthreads();
  sortblk::sort<F2_MAX>(s_key, s_tag, n, S, spill);
  for (int i = threadIdx.x; i < n; i += 256) perm[i] = s_tag[i];
}

// Stages E - G of the CLASSES forms (lmx_ctx_collect_clusters_classes): the chain below per class, as lmx_cluster_matches_classes composes
// it on the host.  The vote key carries the class on top -- class 4 bits | y / step 16 | x / step 16 | ring 17 | list position 11, all
// offset-binary; x and y come from a short, so with step >= 1 sixteen bits lose nothing -- and step, ring constants, size threshold and
// side-car are the class's own (p.classes).  A match whose class has no side-car gets the all-ones key of the padding and is left out of
// the runs; n_valid counts the others, since class 15 at y = x = 32767, ring 2^16 - 1, position 2047 has that key too.  The emulated
// std::sort by score and the greedy NMS take ONE class's clusters at a time (libstdc++'s order of ties depends on the array it sorts, so
// sorting the joined list would not be the composition), and the classes' survivors are written one class after the other.
// s_valid and s_bad are the two LDS words stages A - D are done with.
template <int MODE>
__device__ __forceinline__ void f2_cluster_classes(const F2Params& p, int frame, int nf, unsigned long long* s_key, const float* s_sim, const int* s_tid,
                                                   const short* s_x, const short* s_y, const unsigned short* s_cls, unsigned short* s_perm,
                                                   unsigned short* s_keep, int* s_valid, int* s_bad, const lmx_depth_diff_t* d_final,
                                                   const lmx_normal_diff_t* n_final, uint32_t* counts) {
  constexpr bool SCORED = MODE != F2_SIMILARITY, NORMAL = MODE == F2_DEPTH_NORMAL;
  constexpr int NMAX = F2_MAX;
  const int tid = threadIdx.x;
  const F2Class* const tab = p.classes;
  if (tid == 0) { *s_valid = 0; *s_bad = 0; }
  __syncthreads();
  int nf2 = 1;
  while (nf2 < nf) nf2 <<= 1;
  for (int j = tid; j < nf2; j += 256) {
    unsigned long long key = ~0ull;
    if (j < nf) {
      const int c = s_cls[j];
      if (c < F2_CLASSES && tab[c].n_templates != 0) {
        const int t = s_tid[j];
        if (t < 0 || (uint32_t)t >= tab[c].n_templates) { atomicOr(s_bad, 1); }
        else {
          const int iy = s_y[j] / tab[c].step, ix = s_x[j] / tab[c].step;
          const float depth = (float)tab[c].dists[t];
          const float ring_step = (float)tab[c].radius_step;
          const int ring = (int)((depth - tab[c].radius_min) / ring_step);   // float - double -> double, / float -> double, like the reference
          const long long fr = (long long)ring + (1 << 16);
          if (fr < 0 || fr >= (1 << 17)) atomicOr(s_bad, 2);
          else {
            key = ((unsigned long long)c << 60) | ((unsigned long long)(iy + (1 << 15)) << 44) | ((unsigned long long)(ix + (1 << 15)) << 28) |
                  ((unsigned long long)fr << 11) | (unsigned long long)j;
            atomicAdd(s_valid, 1);
          }
        }
      }
    }
    s_key[j] = key;
  }
  __syncthreads();
  if (*s_bad) {   // a template id outside its class's side-car / a ring outside the packed range: host path
    if (tid == 0) { counts[0] = (uint32_t)nf; counts[1] = 0; counts[2] = 0; counts[3] = 2; }
    return;
  }
  bitonic_sort_u64(s_key, nf2, tid, 256);
  if (tid == 0) {
    const int nv = *s_valid;   // the sorted keys 0 .. nv - 1 are the matches that vote
    lmx_cluster_t* out_c = p.out_clusters + (size_t)frame * NMAX;
    int32_t* out_cls = p.out_cluster_class + (size_t)frame * NMAX;
    int32_t* out_mem = p.out_members + (size_t)frame * NMAX;
    double* c_score = reinterpret_cast<double*>(p.scratch + (size_t)frame * NMAX * 32);
    unsigned long long* c_range = reinterpret_cast<unsigned long long*>(p.scratch + (size_t)frame * NMAX * 32 + (size_t)NMAX * 8);   // begin << 32 | count
    int* c_rect = reinterpret_cast<int*>(p.scratch + (size_t)frame * NMAX * 32 + (size_t)NMAX * 16);
    int n_out = 0, n_mem = 0;
    for (int b = 0; b < nv;) {
      // F for the class whose key range starts at b: its clusters are the runs of equal key up to the next class
      const int c = (int)(s_key[b] >> 60);
      const int size_thresh = tab[c].size_thresh;
      const int32_t* const rects = tab[c].rects;
      int nc = 0;
      while (b < nv && (int)(s_key[b] >> 60) == c) {
        int e = b + 1;
        while (e < nv && (s_key[e] >> 11) == (s_key[b] >> 11)) ++e;
        const int cnt = e - b;
        if (cnt > size_thresh) {
          double sum = 0.0;
          int X = 0, Y = 0, Wd = 0, Ht = 0;
          for (int k = b; k < e; ++k) {
            const int j = (int)(s_key[k] & 2047u);
            if constexpr (NORMAL) sum += nv::value(d_final[j], n_final[j], p.no_value);
            else if constexpr (SCORED) sum += dv::value(d_final[j], p.no_value);
            else sum += (double)s_sim[j];
            const int32_t* r = rects + (size_t)s_tid[j] * 4;
            X += s_x[j]; Y += s_y[j]; Wd += r[2]; Ht += r[3];
          }
          c_range[nc] = ((unsigned long long)b << 32) | (unsigned)cnt;
          c_score[nc] = sum / cnt;
          c_rect[4 * nc + 0] = div_by_size(X, cnt); c_rect[4 * nc + 1] = div_by_size(Y, cnt);
          c_rect[4 * nc + 2] = div_by_size(Wd, cnt); c_rect[4 * nc + 3] = div_by_size(Ht, cnt);
          ++nc;
        }
        b = e;
      }
      // G on this class's clusters alone
      for (int i = 0; i < nc; ++i) { s_perm[i] = (unsigned short)i; s_keep[i] = 0; }
      sortemu::sort(s_perm, nc, [&](unsigned short a, unsigned short b2) { return c_score[a] > c_score[b2]; });
      for (int a = 0; a < nc; ++a) {
        if (s_keep[s_perm[a]]) continue;
        for (int q = a + 1; q < nc; ++q)
          if (!s_keep[s_perm[q]]) {
            const double v = (double)box_iou(&c_rect[4 * s_perm[a]], &c_rect[4 * s_perm[q]]);
            if (v > 0.4) s_keep[s_perm[q]] = 1;
          }
      }
      for (int a = 0; a < nc; ++a) {
        const int ci = s_perm[a];
        if (s_keep[ci]) continue;
        const int first = (int)(c_range[ci] >> 32), cnt = (int)(c_range[ci] & 0xffffffffu);
        lmx_cluster_t o;
        const unsigned long long key = s_key[first];
        o.index[0] = (int)((key >> 44) & 0xffff) - (1 << 15);
        o.index[1] = (int)((key >> 28) & 0xffff) - (1 << 15);
        o.index[2] = (int)((key >> 11) & 0x1ffff) - (1 << 16);
        for (int k = 0; k < 4; ++k) o.rect[k] = c_rect[4 * ci + k];
        o.score = c_score[ci];
        o.member_begin = n_mem; o.member_count = cnt;
        for (int k = first; k < first + cnt; ++k) out_mem[n_mem++] = (int32_t)(s_key[k] & 2047u);
        out_cls[n_out] = c;
        out_c[n_out++] = o;
      }
    }
    counts[0] = (uint32_t)nf; counts[1] = (uint32_t)n_out; counts[2] = (uint32_t)n_mem; counts[3] = 0;
  }
}

template <int MODE, bool CLASSES = false>
__device__ __forceinline__ void f2_finalize_cluster(const F2Params& p) {
  constexpr bool SCORED = MODE != F2_SIMILARITY, NORMAL = MODE == F2_DEPTH_NORMAL;
  constexpr int NMAX = F2_MAX;
  constexpr int PER = (NMAX + 255) / 256;   // items per thread
  __shared__ unsigned long long s_key[NMAX];
  __shared__ float s_sim[NMAX];
  __shared__ int s_tid[NMAX];
  __shared__ short s_x[NMAX], s_y[NMAX];     // image coordinates (< 32768: lmx_bank_add_class validates feature ranges, frames are smaller)
  __shared__ unsigned short s_cls[NMAX];
  __shared__ unsigned short s_perm[NMAX], s_keep[NMAX];   // 52 KB of LDS up to here
  __shared__ unsigned short s_seg[NMAX], s_rpos[NMAX];    // stage C (sortblk::sort; s_keep doubles as its lpos): 64 KB with its range tables
  __shared__ uint32_t s_cut[NMAX / 32];
  __shared__ sortblk::Scratch S;
  __shared__ int s_n, s_nfinal;
  const int tid = threadIdx.x, frame = blockIdx.x;
  uint32_t* counts = p.out_counts + (size_t)frame * 4;
  lmx_match_t* out_m = p.out_matches + (size_t)frame * NMAX;
  // SCORED: this frame's diffs by insertion position (written at the load step, read at the compaction) and by final position (written
  // there, read by lane 0 in F); each read has a __syncthreads() between it and the write
  lmx_depth_diff_t* const d_parked = SCORED ? p.diff_scratch + (size_t)frame * 2 * NMAX : nullptr;
  lmx_depth_diff_t* const d_final = SCORED ? d_parked + NMAX : nullptr;
  lmx_normal_diff_t* const n_parked = NORMAL ? p.ndiff_scratch + (size_t)frame * 2 * NMAX : nullptr;   // the same two rows for the normal sums
  lmx_normal_diff_t* const n_final = NORMAL ? n_parked + NMAX : nullptr;
  if (tid == 0) { s_n = 0; s_nfinal = 0; }
  __syncthreads();
  // A: this frame's records (order arbitrary), identified by their index in the slot's list
  const uint32_t n_total = min(p.hdr[1], p.cap);
  for (uint32_t i = tid; i < n_total; i += 256)
    if (p.recs[i].frame == frame) {
      const int pos = atomicAdd(&s_n, 1);
      if (pos < NMAX) { s_key[pos] = p.recs[i].order_key; s_tid[pos] = (int)i; }   // s_tid borrowed: record index
    }
  __syncthreads();
  const int n = s_n;
  if (n > NMAX) {   // too many for the LDS path: the host finishes this frame
    if (tid == 0) { counts[0] = (uint32_t)n; counts[1] = 0; counts[2] = 0; counts[3] = 1; }
    return;
  }
  // B: insertion order.  order_key is unique per record (class slot | template_id | coarse raster index), so the low bits of
  // a 64-bit key cannot carry the record index; sort (key) and recover the record by a second lookup table: pack the record's
  // LDS position instead -- positions < 2048 need 11 bits, order_key uses 48 + ... bits, so sort pairs through two passes:
  // keys are unique, hence sorting keys alone and locating each record by binary search of its key is exact.
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  unsigned long long my_key[PER];   // this thread's unsorted keys (slots tid, tid + 256, ...)
  {
    int cnt = 0;
    for (int i = tid; i < n2; i += 256, ++cnt) my_key[cnt] = i < n ? s_key[i] : ~0ull;
    __syncthreads();
    cnt = 0;
    for (int i = tid; i < n2; i += 256, ++cnt) s_key[i] = my_key[cnt];
  }
  __syncthreads();
  bitonic_sort_u64(s_key, n2, tid, 256);
  // rank of every record = position of its key in the sorted keys
  {
    int cnt = 0;
    for (int i = tid; i < n; i += 256, ++cnt) {
      const unsigned long long k = my_key[cnt];
      int lo = 0, hi = n - 1;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_key[mid] < k) lo = mid + 1; else hi = mid; }
      s_perm[lo] = (unsigned short)i;   // insertion position lo holds LDS slot i
    }
  }
  __syncthreads();
  // load the records in insertion order
  {
    int rec_of_pos[PER];
    int cnt = 0;
    for (int i = tid; i < n; i += 256) rec_of_pos[cnt++] = s_tid[s_perm[i]];
    __syncthreads();
    cnt = 0;
    for (int i = tid; i < n; i += 256) {
      const lmx_raw_match_t r = p.recs[rec_of_pos[cnt]];
      if constexpr (SCORED) d_parked[i] = p.diffs[rec_of_pos[cnt]];
      if constexpr (NORMAL) n_parked[i] = p.ndiffs[rec_of_pos[cnt]];
      ++cnt;
      s_sim[i] = r.similarity; s_tid[i] = r.template_id; s_x[i] = (short)r.x; s_y[i] = (short)r.y; s_cls[i] = (unsigned short)r.class_index;
    }
  }
  __syncthreads();
  // C: std::sort with Match::operator<, order of ties as libstdc++ leaves it (s_key is free again: the insertion order is in place)
  if (tid == 0) { S.seg = s_seg; S.lpos = s_keep; S.rpos = s_rpos; S.cut_bits = s_cut; }
  for (int i = tid; i < n; i += 256) { s_key[i] = match_sort_key(s_sim[i], s_tid[i]); s_perm[i] = (unsigned short)i; }
  __syncthreads();
  sortblk::sort<NMAX>(s_key, s_perm, n, S, reinterpret_cast<unsigned long long*>(p.scratch + (size_t)frame * NMAX * 32));
  // D: std::unique.  Thread t owns positions t * PER .. t * PER + PER - 1; the kept elements' output positions come from a block scan
  {
    uint32_t kf[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int j = tid * PER + q;
      bool keep = j < n;
      if (keep && j > 0) {
        const int a = s_perm[j - 1], b = s_perm[j];
        keep = !(s_x[a] == s_x[b] && s_y[a] == s_y[b] && s_sim[a] == s_sim[b] && s_cls[a] == s_cls[b]);
      }
      kf[q] = keep ? 1u : 0u;
    }
    uint32_t sc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) sc[q] = kf[q];
    sortblk::block_scan_inclusive<PER>(sc, S.wave_sum, tid);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int j = tid * PER + q;
      if (j < n) s_keep[j] = (unsigned short)(kf[q] ? sc[q] - 1u : 0xffffu);
      if (j == n - 1) s_nfinal = (int)sc[q];
    }
  }
  __syncthreads();
  const int nf = s_nfinal;
  // final list -> global, and compact the LDS arrays into final order (through registers: in-place permutation)
  {
    float r_sim[PER]; int r_tid[PER], r_x[PER], r_y[PER], r_cls[PER], r_dst[PER];
    int cnt = 0;
    for (int j = tid; j < n; j += 256, ++cnt) {
      const int src = s_perm[j];
      r_dst[cnt] = s_keep[j] == 0xffff ? -1 : (int)s_keep[j];
      r_sim[cnt] = s_sim[src]; r_tid[cnt] = s_tid[src]; r_x[cnt] = s_x[src]; r_y[cnt] = s_y[src]; r_cls[cnt] = s_cls[src];
    }
    __syncthreads();
    cnt = 0;
    for (int j = tid; j < n; j += 256, ++cnt) {
      const int d = r_dst[cnt];
      if (d < 0) continue;
      s_sim[d] = r_sim[cnt]; s_tid[d] = r_tid[cnt]; s_x[d] = (short)r_x[cnt]; s_y[d] = (short)r_y[cnt]; s_cls[d] = (unsigned short)r_cls[cnt];
      lmx_match_t m;
      m.x = r_x[cnt]; m.y = r_y[cnt]; m.similarity = r_sim[cnt]; m.template_id = r_tid[cnt]; m.class_index = r_cls[cnt];
      out_m[d] = m;
      if constexpr (SCORED) {
        const lmx_depth_diff_t dd = d_parked[s_perm[j]];   // s_perm is not touched by this step
        d_final[d] = dd;
        p.out_diffs[(size_t)frame * NMAX + d] = dd;
      }
      if constexpr (NORMAL) {
        const lmx_normal_diff_t nd = n_parked[s_perm[j]];
        n_final[d] = nd;
        p.out_ndiffs[(size_t)frame * NMAX + d] = nd;
      }
    }
  }
  __syncthreads();
  if (!p.do_clusters) {
    if (tid == 0) { counts[0] = (uint32_t)nf; counts[1] = 0; counts[2] = 0; counts[3] = 0; }
    return;
  }
  if constexpr (CLASSES) {   // E - G per class, on the same LDS
    f2_cluster_classes<MODE>(p, frame, nf, s_key, s_sim, s_tid, s_x, s_y, s_cls, s_perm, s_keep, &s_n, &s_nfinal, d_final, n_final, counts);
    return;
  }
  // E: rcd_voting keys.  {y / step, x / step, ring} compared lexicographically as signed ints (std::map<vector<int>, ...>):
  // offset-binary fields of 17 + 17 + 19 bits, the match's position in the final list in the low 11 bits (keeps the order in
  // which matches were voted into a bin)
  __shared__ int s_bad;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  int nf2 = 1;
  while (nf2 < nf) nf2 <<= 1;
  for (int j = tid; j < nf2; j += 256) {
    unsigned long long key = ~0ull;
    if (j < nf) {
      const int t = s_tid[j];
      if (t < 0 || (uint32_t)t >= p.n_templates) { atomicOr(&s_bad, 1); }
      else {
        const int iy = s_y[j] / p.step, ix = s_x[j] / p.step;
        const float depth = (float)p.dists[t];
        const float ring_step = (float)p.radius_step;
        const int ring = (int)((depth - p.radius_min) / ring_step);   // float - double -> double, / float -> double, like the reference
        const long long fy = (long long)iy + (1 << 16), fx = (long long)ix + (1 << 16), fr = (long long)ring + (1 << 18);
        if (fy < 0 || fy >= (1 << 17) || fx < 0 || fx >= (1 << 17) || fr < 0 || fr >= (1 << 19)) atomicOr(&s_bad, 2);
        else key = ((unsigned long long)fy << 47) | ((unsigned long long)fx << 30) | ((unsigned long long)fr << 11) | (unsigned long long)j;
      }
    }
    s_key[j] = key;
  }
  __syncthreads();
  if (s_bad) {   // side-car too short / indices outside the packed range: host path
    if (tid == 0) { counts[0] = (uint32_t)nf; counts[1] = 0; counts[2] = 0; counts[3] = 2; }
    return;
  }
  bitonic_sort_u64(s_key, nf2, tid, 256);
  // F + G on one lane: cluster runs, filter, scores, rects, std::sort by score, greedy NMS
  if (tid == 0) {
    lmx_cluster_t* out_c = p.out_clusters + (size_t)frame * NMAX;
    int32_t* out_mem = p.out_members + (size_t)frame * NMAX;
    // clusters in std::map order = runs of equal key in the sorted array; per-cluster attributes go to a global scratch area
    // (score, range, rect: 8 + 8 + 16 bytes per cluster), order and suppression flags to the LDS arrays that are free now
    int nc = 0;
    double* c_score = reinterpret_cast<double*>(p.scratch + (size_t)frame * NMAX * 32);
    unsigned long long* c_range = reinterpret_cast<unsigned long long*>(p.scratch + (size_t)frame * NMAX * 32 + (size_t)NMAX * 8);   // begin << 32 | count
    int* c_rect = reinterpret_cast<int*>(p.scratch + (size_t)frame * NMAX * 32 + (size_t)NMAX * 16);
    for (int b = 0; b < nf;) {
      int e = b + 1;
      while (e < nf && (s_key[e] >> 11) == (s_key[b] >> 11)) ++e;
      const int cnt = e - b;
      if (cnt > p.size_thresh) {   // cluster_filter: drop clusters with size <= thresh
        double sum = 0.0;
        int X = 0, Y = 0, Wd = 0, Ht = 0;
        for (int k = b; k < e; ++k) {
          const int j = (int)(s_key[k] & 2047u);
          if constexpr (NORMAL) sum += nv::value(d_final[j], n_final[j], p.no_value);
          else if constexpr (SCORED) sum += dv::value(d_final[j], p.no_value);
          else sum += (double)s_sim[j];
          const int32_t* r = p.rects + (size_t)s_tid[j] * 4;
          X += s_x[j]; Y += s_y[j]; Wd += r[2]; Ht += r[3];
        }
        c_range[nc] = ((unsigned long long)b << 32) | (unsigned)cnt;
        c_score[nc] = sum / cnt;
        // upstream: `int X; ... X /= matches.size();` -- the int is converted to size_t for the division (src/rgbdDetector.cpp:
        // nonMaximaSuppressionUsingIOU), so a NEGATIVE sum (matches left of / above the image origin) divides as 2^64 + X
        c_rect[4 * nc + 0] = div_by_size(X, cnt); c_rect[4 * nc + 1] = div_by_size(Y, cnt);
        c_rect[4 * nc + 2] = div_by_size(Wd, cnt); c_rect[4 * nc + 3] = div_by_size(Ht, cnt);
        ++nc;
      }
      b = e;
    }
    for (int i = 0; i < nc; ++i) { s_perm[i] = (unsigned short)i; s_keep[i] = 0; }
    sortemu::sort(s_perm, nc, [&](unsigned short a, unsigned short b) { return c_score[a] > c_score[b]; });
    for (int a = 0; a < nc; ++a) {
      if (s_keep[s_perm[a]]) continue;
      for (int b = a + 1; b < nc; ++b)
        if (!s_keep[s_perm[b]]) {
          const double v = (double)box_iou(&c_rect[4 * s_perm[a]], &c_rect[4 * s_perm[b]]);
          if (v > 0.4) s_keep[s_perm[b]] = 1;
        }
    }
    int n_out = 0, n_mem = 0;
    for (int a = 0; a < nc; ++a) {
      const int c = s_perm[a];
      if (s_keep[c]) continue;
      const int b = (int)(c_range[c] >> 32), cnt = (int)(c_range[c] & 0xffffffffu);
      lmx_cluster_t o;
      const unsigned long long key = s_key[b];
      o.index[0] = (int)((key >> 47) & 0x1ffff) - (1 << 16);
      o.index[1] = (int)((key >> 30) & 0x1ffff) - (1 << 16);
      o.index[2] = (int)((key >> 11) & 0x7ffff) - (1 << 18);
      for (int k = 0; k < 4; ++k) o.rect[k] = c_rect[4 * c + k];
      o.score = c_score[c];
      o.member_begin = n_mem; o.member_count = cnt;
      for (int k = b; k < b + cnt; ++k) out_mem[n_mem++] = (int32_t)(s_key[k] & 2047u);
      out_c[n_out++] = o;
    }
    counts[0] = (uint32_t)nf; counts[1] = (uint32_t)n_out; counts[2] = (uint32_t)n_mem; counts[3] = 0;
  }
}

// every instantiation as a kernel of its own
template <int MODE, bool CLASSES>
__global__ __launch_bounds__(256) void k_f2_finalize_cluster(F2Params p) { f2_finalize_cluster<MODE, CLASSES>(p); }

// ---- the large-frame form: frames of F2_MAX + 1 .. F2_LARGE_MAX records ------------------------------------------------------------------
// The same stages with the same semantics and the same order of ties, for the frames the kernels above hand back with status 1.  What
// changes is where the data lives and which stages run on one lane:
//   * one workgroup of 1024 threads per listed frame; every per-record row (keys, tags, the match fields, the sort's seg / lpos / rpos)
//     lies in the frame's part of a device-memory workspace (F2LargeLayout) that only this workgroup touches, every write separated from
//     its reads by a __syncthreads().  LDS holds what is small and hot: the sort's per-range tables (1024 ranges), the cut bits and stage
//     G's scores, order and suppression flags for up to F2L_GCAP clusters of a class (more: the workspace, on the same code);
//   * the final list is written to the workspace once (out_matches, out_diffs, out_ndiffs) and stages E - G read it there: no parked and
//     no final copy of the diffs;
//   * F gives every run of equal vote key one thread, which sums its members sequentially in voted order (the double sum's order is
//     observable); block scans find the runs and compact the surviving clusters in std::map order;
//   * G keeps the sequential std::sort restatement on one lane (on LDS) and the sequential greedy loop over a; the suppression tests of
//     all q > a of a kept a go across the workgroup; a block scan places the survivors and their member ranges;
//   * vote keys carry a 14-bit list position: y / step 16 | x / step 16 | ring 18 | position 14 (x and y come from a short, so 16 bits
//     lose nothing for step >= 1), classed: class 4 | y / step 16 | x / step 16 | ring 14 | position 14.  A ring outside +-2^17 (classed:
//     +-2^13) gives status 2, as a ring outside the small kernels' range does there;
//   * depth limit reached (median-of-three killers): the remaining ranges are heap-sorted one per thread, as above -- slow on device
//     memory (tens of milliseconds for a 16384-record killer), exact, and no input a matcher produces.
constexpr int F2L_T = 1024;
constexpr int F2L_GCAP = 4096;   // clusters of one class whose stage G runs on LDS
using F2LScratch = sortblk::ScratchT<1024, F2L_T>;

struct F2LRows {   // one frame's part of the workspace
  lmx_match_t* out_m; lmx_cluster_t* out_c; int32_t* out_mem; int32_t* out_cls; lmx_depth_diff_t* out_d; lmx_normal_diff_t* out_n;
  unsigned long long *key, *spill, *c_range; double* c_score; int* c_rect;
  float* sim; int *tid, *rec; short *x, *y; unsigned short *cls, *perm, *keep, *seg, *rpos;
};
__device__ __forceinline__ F2LRows f2l_rows(uint8_t* w, const F2LargeLayout& l) {
  F2LRows r;
  r.out_m = reinterpret_cast<lmx_match_t*>(w + l.matches); r.out_c = reinterpret_cast<lmx_cluster_t*>(w + l.clusters);
  r.out_mem = reinterpret_cast<int32_t*>(w + l.members); r.out_cls = reinterpret_cast<int32_t*>(w + l.cluster_class);
  r.out_d = reinterpret_cast<lmx_depth_diff_t*>(w + l.diffs); r.out_n = reinterpret_cast<lmx_normal_diff_t*>(w + l.ndiffs);
  r.key = reinterpret_cast<unsigned long long*>(w + l.key); r.spill = reinterpret_cast<unsigned long long*>(w + l.spill);
  r.c_range = reinterpret_cast<unsigned long long*>(w + l.c_range); r.c_score = reinterpret_cast<double*>(w + l.c_score);
  r.c_rect = reinterpret_cast<int*>(w + l.c_rect);
  r.sim = reinterpret_cast<float*>(w + l.sim); r.tid = reinterpret_cast<int*>(w + l.tid); r.rec = reinterpret_cast<int*>(w + l.rec);
  r.x = reinterpret_cast<short*>(w + l.x); r.y = reinterpret_cast<short*>(w + l.y);
  r.cls = reinterpret_cast<unsigned short*>(w + l.cls); r.perm = reinterpret_cast<unsigned short*>(w + l.perm);
  r.keep = reinterpret_cast<unsigned short*>(w + l.keep); r.seg = reinterpret_cast<unsigned short*>(w + l.seg);
  r.rpos = reinterpret_cast<unsigned short*>(w + l.rpos);
  return r;
}

// test hook (lmx_debug_device_sort_perm_large): the permutation sortblk::sort produces for n <= F2_LARGE_MAX pairs, on the rows and with
// the scratch the large kernel gives it
__global__ __launch_bounds__(F2L_T) void k_debug_block_sort_large(const float* sim, const int* tid_in, int n, int* perm, uint8_t* ws, F2LargeLayout lay) {
  __shared__ F2LScratch S;
  __shared__ uint32_t s_cut[F2_LARGE_MAX / 32];
  const F2LRows r = f2l_rows(ws, lay);
  if (threadIdx.x == 0) { S.seg = r.seg; S.lpos = r.keep; S.rpos = r.rpos; S.cut_bits = s_cut; }
  for (int i = threadIdx.x; i < n; i += F2L_T) { r.key[i] = match_sort_key(sim[i], tid_in[i]); r.perm[i] = (unsigned short)i; }
  __syncthreads();
  sortblk::sort<F2_LARGE_MAX>(r.key, r.perm, n, S, r.spill);
  for (int i = threadIdx.x; i < n; i += F2L_T) perm[i] = r.perm[i];
}

template <int MODE, bool CLASSES>
__device__ __forceinline__ void f2_large(const F2LargeParams& lp) {
  constexpr bool SCORED = MODE != F2_SIMILARITY, NORMAL = MODE == F2_DEPTH_NORMAL;
  constexpr int NMAX = F2_LARGE_MAX, T = F2L_T;
  constexpr int PER = NMAX / T;   // items per thread where a thread owns a block of positions
  constexpr int POS = 14;         // bits of a match's list position in a vote key
  constexpr unsigned POS_MASK = (1u << POS) - 1u;
  __shared__ F2LScratch S;
  __shared__ uint32_t s_cut[NMAX / 32];
  __shared__ double s_gscore[F2L_GCAP];
  __shared__ unsigned short s_gperm[F2L_GCAP], s_gsup[F2L_GCAP];
  __shared__ int s_n, s_nfinal, s_bad, s_valid, s_total, s_cbegin[F2_CLASSES + 1];
  const F2Params& p = lp.p;
  if (lp.n_listed && blockIdx.x >= *lp.n_listed) return;   // a list built on the device: the grid is its capacity (the whole workgroup leaves)
  const int tid = threadIdx.x, frame = lp.frames[blockIdx.x];
  const F2LRows r = f2l_rows(lp.ws + (size_t)blockIdx.x * lp.lay.bytes, lp.lay);
  uint32_t* counts = p.out_counts + (size_t)blockIdx.x * 4;
  const F2Class* const tab = p.classes;
  if (tid == 0) { s_n = 0; s_nfinal = 0; s_bad = 0; s_valid = 0; }
  __syncthreads();
  // A: this frame's records (order arbitrary), identified by their index in the slot's list
  const uint32_t n_total = min(p.hdr[1], p.cap);
  for (uint32_t i = tid; i < n_total; i += T)
    if (p.recs[i].frame == frame) {
      const int pos = atomicAdd(&s_n, 1);
      if (pos < NMAX) { r.key[pos] = p.recs[i].order_key; r.rec[pos] = (int)i; }
    }
  __syncthreads();
  const int n = s_n;
  if (n > NMAX) {   // the host finishes this frame
    if (tid == 0) { counts[0] = (uint32_t)n; counts[1] = 0; counts[2] = 0; counts[3] = 1; }
    return;
  }
  // B: insertion order.  The keys are unique: sort them alone and find each record's rank by binary search of its key (kept in spill)
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int i = tid; i < n2; i += T) {
    if (i < n) r.spill[i] = r.key[i];
    else r.key[i] = ~0ull;
  }
  __syncthreads();
  bitonic_sort_u64(r.key, n2, tid, T);
  for (int i = tid; i < n; i += T) {
    const unsigned long long k = r.spill[i];
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (r.key[mid] < k) lo = mid + 1; else hi = mid; }
    r.perm[lo] = (unsigned short)i;   // insertion position lo holds arrival slot i
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) r.tid[i] = r.rec[r.perm[i]];   // record index by insertion position (tid borrowed)
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    const int ri = r.tid[i];
    const lmx_raw_match_t m = p.recs[ri];
    r.rec[i] = ri;
    r.sim[i] = m.similarity; r.tid[i] = m.template_id; r.x[i] = (short)m.x; r.y[i] = (short)m.y; r.cls[i] = (unsigned short)m.class_index;
  }
  __syncthreads();
  // C: std::sort with Match::operator<, order of ties as libstdc++ leaves it
  if (tid == 0) { S.seg = r.seg; S.lpos = r.keep; S.rpos = r.rpos; S.cut_bits = s_cut; }
  for (int i = tid; i < n; i += T) { r.key[i] = match_sort_key(r.sim[i], r.tid[i]); r.perm[i] = (unsigned short)i; }
  __syncthreads();
  sortblk::sort<NMAX>(r.key, r.perm, n, S, r.spill);
  // D: std::unique.  Thread t owns positions t * PER .. t * PER + PER - 1; the kept elements' output positions come from a block scan
  {
    uint32_t kf[PER], sc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int j = tid * PER + q;
      bool keep = j < n;
      if (keep && j > 0) {
        const int a = r.perm[j - 1], b = r.perm[j];
        keep = !(r.x[a] == r.x[b] && r.y[a] == r.y[b] && r.sim[a] == r.sim[b] && r.cls[a] == r.cls[b]);
      }
      kf[q] = keep ? 1u : 0u;
      sc[q] = kf[q];
    }
    sortblk::block_scan_inclusive<PER>(sc, S.wave_sum, tid);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int j = tid * PER + q;
      if (j < n) r.keep[j] = (unsigned short)(kf[q] ? sc[q] - 1u : 0xffffu);
      if (j == n - 1) s_nfinal = (int)sc[q];
    }
  }
  __syncthreads();
  const int nf = s_nfinal;
  // the final list, with each match's diffs next to it: written once, read by E - G
  for (int j = tid; j < n; j += T) {
    const int d = r.keep[j];
    if (d == 0xffff) continue;
    const int src = r.perm[j];
    lmx_match_t m;
    m.x = r.x[src]; m.y = r.y[src]; m.similarity = r.sim[src]; m.template_id = r.tid[src]; m.class_index = r.cls[src];
    r.out_m[d] = m;
    if constexpr (SCORED) r.out_d[d] = p.diffs[r.rec[src]];
    if constexpr (NORMAL) r.out_n[d] = p.ndiffs[r.rec[src]];
  }
  __syncthreads();
  if (!p.do_clusters) {
    if (tid == 0) { counts[0] = (uint32_t)nf; counts[1] = 0; counts[2] = 0; counts[3] = 0; }
    return;
  }
  // E: rcd_voting keys, offset-binary fields; padding and (classed) matches whose class has no side-car get the all-ones key
  int nf2 = 1;
  while (nf2 < nf) nf2 <<= 1;
  for (int j = tid; j < nf2; j += T) {
    unsigned long long key = ~0ull;
    if (j < nf) {
      const lmx_match_t m = r.out_m[j];
      const int t = m.template_id;
      if constexpr (CLASSES) {
        const int c = m.class_index;
        if (c < F2_CLASSES && tab[c].n_templates != 0) {
          if (t < 0 || (uint32_t)t >= tab[c].n_templates) atomicOr(&s_bad, 1);
          else {
            const int iy = m.y / tab[c].step, ix = m.x / tab[c].step;
            const float depth = (float)tab[c].dists[t];
            const float ring_step = (float)tab[c].radius_step;
            const int ring = (int)((depth - tab[c].radius_min) / ring_step);   // float - double -> double, / float -> double, like the reference
            const long long fr = (long long)ring + (1 << 13);
            if (fr < 0 || fr >= (1 << 14)) atomicOr(&s_bad, 2);
            else {
              key = ((unsigned long long)c << 60) | ((unsigned long long)(iy + (1 << 15)) << 44) | ((unsigned long long)(ix + (1 << 15)) << 28) |
                    ((unsigned long long)fr << POS) | (unsigned long long)j;
              atomicAdd(&s_valid, 1);
            }
          }
        }
      } else {
        if (t < 0 || (uint32_t)t >= p.n_templates) atomicOr(&s_bad, 1);
        else {
          const int iy = m.y / p.step, ix = m.x / p.step;
          const float depth = (float)p.dists[t];
          const float ring_step = (float)p.radius_step;
          const int ring = (int)((depth - p.radius_min) / ring_step);
          const long long fr = (long long)ring + (1 << 17);
          if (fr < 0 || fr >= (1 << 18)) atomicOr(&s_bad, 2);
          else key = ((unsigned long long)(iy + (1 << 15)) << 48) | ((unsigned long long)(ix + (1 << 15)) << 32) | ((unsigned long long)fr << POS) | (unsigned long long)j;
        }
      }
    }
    r.key[j] = key;
  }
  __syncthreads();
  if (s_bad) {   // side-car too short / ring outside the packed range: host path
    if (tid == 0) { counts[0] = (uint32_t)nf; counts[1] = 0; counts[2] = 0; counts[3] = 2; }
    return;
  }
  bitonic_sort_u64(r.key, nf2, tid, T);
  const int nv = CLASSES ? s_valid : nf;   // the sorted keys 0 .. nv - 1 are the matches that vote
  // F: clusters in std::map order = runs of equal key above the position bits.  Run starts (seg is free again), then the runs that pass
  // cluster_filter compacted in order, then one thread per surviving run
  unsigned short* const run_start = r.seg;
  {
    uint32_t fl[PER], sc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int k = tid * PER + q;
      fl[q] = (k < nv && (k == 0 || (r.key[k] >> POS) != (r.key[k - 1] >> POS))) ? 1u : 0u;
      sc[q] = fl[q];
    }
    sortblk::block_scan_inclusive<PER>(sc, S.wave_sum, tid);
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (fl[q]) run_start[sc[q] - 1u] = (unsigned short)(tid * PER + q);
    if (tid == T - 1) s_total = (int)sc[PER - 1];
  }
  __syncthreads();
  const int n_runs = s_total;
  __syncthreads();
  {
    uint32_t fl[PER], sc[PER], rb[PER], rc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int k = tid * PER + q;
      fl[q] = 0; rb[q] = 0; rc[q] = 0;
      if (k < n_runs) {
        rb[q] = run_start[k];
        rc[q] = (uint32_t)(k + 1 < n_runs ? run_start[k + 1] : nv) - rb[q];
        const int thresh = CLASSES ? tab[r.key[rb[q]] >> 60].size_thresh : p.size_thresh;
        fl[q] = (int)rc[q] > thresh ? 1u : 0u;   // cluster_filter: drop clusters with size <= thresh
      }
      sc[q] = fl[q];
    }
    sortblk::block_scan_inclusive<PER>(sc, S.wave_sum, tid);
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (fl[q]) r.c_range[sc[q] - 1u] = ((unsigned long long)rb[q] << 32) | rc[q];   // begin << 32 | count
    if (tid == T - 1) s_total = (int)sc[PER - 1];
    if (tid <= F2_CLASSES) s_cbegin[tid] = -1;
  }
  __syncthreads();
  const int nc = s_total;
  for (int ci = tid; ci < nc; ci += T) {
    const int b = (int)(r.c_range[ci] >> 32), cnt = (int)(r.c_range[ci] & 0xffffffffu);
    const int32_t* rects = p.rects;
    if constexpr (CLASSES) {
      const int c = (int)(r.key[b] >> 60);
      rects = tab[c].rects;
      if (ci == 0 || (int)(r.key[(int)(r.c_range[ci - 1] >> 32)] >> 60) != c) s_cbegin[c] = ci;   // the class's first cluster
    }
    double sum = 0.0;
    int X = 0, Y = 0, Wd = 0, Ht = 0;
    for (int k = b; k < b + cnt; ++k) {
      const int j = (int)(r.key[k] & POS_MASK);
      const lmx_match_t m = r.out_m[j];
      if constexpr (NORMAL) sum += nv::value(r.out_d[j], r.out_n[j], p.no_value);
      else if constexpr (SCORED) sum += dv::value(r.out_d[j], p.no_value);
      else sum += (double)m.similarity;
      const int32_t* rr = rects + (size_t)m.template_id * 4;
      X += m.x; Y += m.y; Wd += rr[2]; Ht += rr[3];
    }
    r.c_score[ci] = sum / cnt;
    // upstream: `int X; ... X /= matches.size();` -- see div_by_size
    r.c_rect[4 * ci + 0] = div_by_size(X, cnt); r.c_rect[4 * ci + 1] = div_by_size(Y, cnt);
    r.c_rect[4 * ci + 2] = div_by_size(Wd, cnt); r.c_rect[4 * ci + 3] = div_by_size(Ht, cnt);
  }
  __syncthreads();
  // G, one class's clusters at a time (un-classed: all of them): std::sort by score on one lane, greedy NMS with the suppression tests
  // of a kept cluster across the workgroup, survivors placed by a block scan
  int n_out = 0, n_mem = 0;
  for (int c = 0; c < (CLASSES ? F2_CLASSES : 1); ++c) {
    int cb = 0, ce = nc;
    if constexpr (CLASSES) {
      cb = s_cbegin[c];
      if (cb < 0) continue;
      for (int c2 = c + 1; c2 < F2_CLASSES; ++c2)
        if (s_cbegin[c2] >= 0) { ce = s_cbegin[c2]; break; }
    }
    const int m = ce - cb;
    if (m <= 0) continue;
    // order and suppression flags: LDS, or the rows the big sort is done with
    double* const gscore = m <= F2L_GCAP ? s_gscore : r.c_score + cb;
    unsigned short* const gperm = m <= F2L_GCAP ? s_gperm : r.perm;
    unsigned short* const gsup = m <= F2L_GCAP ? s_gsup : r.keep;
    const int* const crect = r.c_rect + 4 * (size_t)cb;
    for (int i = tid; i < m; i += T) {
      if (m <= F2L_GCAP) gscore[i] = r.c_score[cb + i];
      gperm[i] = (unsigned short)i; gsup[i] = 0;
    }
    __syncthreads();
    if (tid == 0) sortemu::sort(gperm, m, [&](unsigned short a, unsigned short b) { return gscore[a] > gscore[b]; });
    __syncthreads();
    for (int a = 0; a < m; ++a) {
      const int pa = gperm[a];
      if (gsup[pa]) continue;   // the same for every thread: flags are written before a barrier, read after it
      for (int q = a + 1 + tid; q < m; q += T) {
        const int pq = gperm[q];
        if (!gsup[pq]) {
          const double v = (double)box_iou(&crect[4 * pa], &crect[4 * pq]);
          if (v > 0.4) gsup[pq] = 1;
        }
      }
      __syncthreads();
    }
    // survivors in sorted order; a thread owns PER consecutive ranks.  One scan of kept << 0 | members << 16 (both <= 16384)
    {
      uint32_t fl[PER], sc[PER];
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int a = tid * PER + q;
        fl[q] = 0;
        if (a < m && !gsup[gperm[a]]) fl[q] = 1u | ((uint32_t)(r.c_range[cb + gperm[a]] & 0xffffffffu) << 16);
        sc[q] = fl[q];
      }
      sortblk::block_scan_inclusive<PER>(sc, S.wave_sum, tid);
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        if (!fl[q]) continue;
        const int ci = cb + gperm[tid * PER + q];
        const int first = (int)(r.c_range[ci] >> 32), cnt = (int)(fl[q] >> 16);
        const int at = n_out + (int)(sc[q] & 0xffffu) - 1, mem_at = n_mem + (int)(sc[q] >> 16) - cnt;
        lmx_cluster_t o;
        const unsigned long long key = r.key[first];
        if constexpr (CLASSES) {
          o.index[0] = (int)((key >> 44) & 0xffff) - (1 << 15);
          o.index[1] = (int)((key >> 28) & 0xffff) - (1 << 15);
          o.index[2] = (int)((key >> POS) & 0x3fff) - (1 << 13);
          r.out_cls[at] = c;
        } else {
          o.index[0] = (int)((key >> 48) & 0xffff) - (1 << 15);
          o.index[1] = (int)((key >> 32) & 0xffff) - (1 << 15);
          o.index[2] = (int)((key >> POS) & 0x3ffff) - (1 << 17);
        }
        for (int k = 0; k < 4; ++k) o.rect[k] = r.c_rect[4 * ci + k];
        o.score = r.c_score[ci];
        o.member_begin = mem_at; o.member_count = cnt;
        for (int k = 0; k < cnt; ++k) r.out_mem[mem_at + k] = (int32_t)(r.key[first + k] & POS_MASK);
        r.out_c[at] = o;
      }
      if (tid == T - 1) s_total = (int)sc[PER - 1];
      __syncthreads();
      n_out += s_total & 0xffff; n_mem += s_total >> 16;
      __syncthreads();
    }
  }
  if (tid == 0) { counts[0] = (uint32_t)nf; counts[1] = (uint32_t)n_out; counts[2] = (uint32_t)n_mem; counts[3] = 0; }
}

template <int MODE, bool CLASSES>
__global__ __launch_bounds__(F2L_T) void k_f2_large(F2LargeParams p) { f2_large<MODE, CLASSES>(p); }

void launch_debug_block_sort_large(hipStream_t s, const float* sim, const int* tid, int n, int* perm, uint8_t* ws) {
  hipLaunchKernelGGL(k_debug_block_sort_large, dim3(1), dim3(F2L_T), 0, s, sim, tid, n, perm, ws, f2_large_layout(F2_SIMILARITY));
}

void launch_f2_large(hipStream_t s, const F2LargeParams& p, int n_listed, F2Score score, bool classes) {
  const dim3 grid((unsigned)n_listed), block(F2L_T);
  switch (2 * score + (classes ? 1 : 0)) {
    case 2 * F2_SIMILARITY: hipLaunchKernelGGL((k_f2_large<F2_SIMILARITY, false>), grid, block, 0, s, p); break;
    case 2 * F2_SIMILARITY + 1: hipLaunchKernelGGL((k_f2_large<F2_SIMILARITY, true>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH: hipLaunchKernelGGL((k_f2_large<F2_DEPTH, false>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH + 1: hipLaunchKernelGGL((k_f2_large<F2_DEPTH, true>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH_NORMAL: hipLaunchKernelGGL((k_f2_large<F2_DEPTH_NORMAL, false>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH_NORMAL + 1: hipLaunchKernelGGL((k_f2_large<F2_DEPTH_NORMAL, true>), grid, block, 0, s, p); break;
  }
}

void launch_debug_block_sort(hipStream_t s, const float* sim, const int* tid, int n, int* perm, unsigned long long* spill) {
  hipLaunchKernelGGL(k_debug_block_sort, dim3(1), dim3(256), 0, s, sim, tid, n, perm, spill);
}

void launch_f2(hipStream_t s, const F2Params& p, F2Score score, bool classes) {
  const dim3 grid((unsigned)p.n_frames), block(256);
  switch (2 * score + (classes ? 1 : 0)) {
    case 2 * F2_SIMILARITY: hipLaunchKernelGGL((k_f2_finalize_cluster<F2_SIMILARITY, false>), grid, block, 0, s, p); break;
    case 2 * F2_SIMILARITY + 1: hipLaunchKernelGGL((k_f2_finalize_cluster<F2_SIMILARITY, true>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH: hipLaunchKernelGGL((k_f2_finalize_cluster<F2_DEPTH, false>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH + 1: hipLaunchKernelGGL((k_f2_finalize_cluster<F2_DEPTH, true>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH_NORMAL: hipLaunchKernelGGL((k_f2_finalize_cluster<F2_DEPTH_NORMAL, false>), grid, block, 0, s, p); break;
    case 2 * F2_DEPTH_NORMAL + 1: hipLaunchKernelGGL((k_f2_finalize_cluster<F2_DEPTH_NORMAL, true>), grid, block, 0, s, p); break;
  }
}

}  // namespace lmx
