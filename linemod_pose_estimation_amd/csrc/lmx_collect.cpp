// liblmx.so, behind the kernel chain: read-back of an output slot and the host finalisation (restore upstream insertion order, then the
// very std::sort / std::unique Detector::match applies), the device-side consumer chain (lmx_ctx_collect_clusters), its
// forms that leave the results in the caller's device memory (lmx_ctx_export_matches_on, lmx_ctx_export_clusters_on), and the multi-GPU plumbing on one context's
// side: gather-block export, copies by kernel, the host merge of gathered blocks.

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "lmx_ctx.hpp"
#include "lmx_depth_verify.hpp"
#include "lmx_normal_verify.hpp"

using namespace lmx;

namespace {

// upstream Match ordering; class identity is the class index
struct HostMatch {
  lmx_match_t m;
  bool operator<(const HostMatch& r) const {
    if (m.similarity != r.m.similarity) return m.similarity > r.m.similarity;
    return m.template_id < r.m.template_id;
  }
  bool operator==(const HostMatch& r) const {
    return m.x == r.m.x && m.y == r.m.y && m.similarity == r.m.similarity && m.class_index == r.m.class_index;
  }
};

// records of ONE frame -> upstream output order.  Insertion order is restored from order_key, then the very
// same std::sort / std::unique upstream applies (libstdc++'s tie order is part of the observable result).
static void finalize_frame(std::vector<const lmx_raw_match_t*>& recs, std::vector<HostMatch>& out) {
  // back into upstream's insertion order (the keys are distinct: one record per class, template and coarse position).  Long lists sort
  // (key, pointer) pairs instead of dereferencing a pointer per comparison: the records lie in pinned memory in arrival order
  if (recs.size() > 4096) {
    std::vector<std::pair<uint64_t, const lmx_raw_match_t*>> keyed(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) keyed[i] = {recs[i]->order_key, recs[i]};
    std::sort(keyed.begin(), keyed.end(), [](const std::pair<uint64_t, const lmx_raw_match_t*>& a, const std::pair<uint64_t, const lmx_raw_match_t*>& b) { return a.first < b.first; });
    for (size_t i = 0; i < recs.size(); ++i) recs[i] = keyed[i].second;
  } else {
    std::sort(recs.begin(), recs.end(), [](const lmx_raw_match_t* a, const lmx_raw_match_t* b) { return a->order_key < b->order_key; });
  }
  out.clear();
  out.reserve(recs.size());
  for (const lmx_raw_match_t* r : recs) {
    HostMatch h;
    h.m.x = r->x; h.m.y = r->y; h.m.similarity = r->similarity; h.m.template_id = r->template_id; h.m.class_index = r->class_index;
    out.push_back(h);
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
}

}  // namespace

extern "C" {

// sync + read-back + per-frame finalisation shared by collect / collect_flat
static lmx_status collect_impl(lmx_ctx* c, int32_t n_frames, std::vector<std::vector<HostMatch>>& fin) {
  if (c->outstanding < 1) { set_error("lmx_ctx_collect: nothing enqueued"); return LMX_ERR_INVALID_ARG; }
  const int slot = (c->head + c->n_slots - c->outstanding) % c->n_slots;  // oldest outstanding enqueue
  if (n_frames != c->slot_frames[slot]) { set_error("lmx_ctx_collect: n_frames=%d but the enqueue had %d", n_frames, c->slot_frames[slot]); return LMX_ERR_INVALID_ARG; }
  LMX_HIP(hipSetDevice(c->device));
  const size_t first = std::min<size_t>(c->h_out_records, lmx_ctx::kFirstSlice);
  using clk = std::chrono::steady_clock;
  const clk::time_point t0 = clk::now();
  bool seen = false;
  if (c->pub_seq[slot] != 0 && !c->env.no_header_poll && c->profiling == 0) {
    // one or two frames per call: k_refine's last workgroup publishes the slot and then its sequence number (word 7 of the pinned header);
    // spinning on that word sees the result a few microseconds before the event's wake-up does.  Bounded: 200 us, then the event as always
    const volatile uint32_t* word = reinterpret_cast<const volatile uint32_t*>(c->h_out_slot[slot]) + 7;
    const uint32_t want = c->pub_seq[slot];
    for (;;) {
      if (*word == want) { seen = true; break; }
      if (clk::now() - t0 > std::chrono::microseconds(200)) break;
      __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  if (!seen) LMX_HIP(hipEventSynchronize(c->done[slot]));
  const clk::time_point t1 = clk::now();
  c->h_out = c->h_out_slot[slot];
  uint8_t* const d_slot = c->d_out_slot[slot];
  if (lmx_status xs = wait_exports(c, slot)) return xs;   // an export may still read the slot this call frees
  c->outstanding -= 1;
  if (c->outstanding == 0) drain_profiling(c);  // every recorded event has completed
  const uint32_t n_cand = reinterpret_cast<uint32_t*>(c->h_out)[0];
  const uint32_t n_match = reinterpret_cast<uint32_t*>(c->h_out)[1];
  if (c->env.debug_collect) {
    // diagnostics: the device-side slot against its pinned host mirror once the slot's event has completed
    uint32_t dev[16];
    if (hipMemcpy(dev, d_slot, 64, hipMemcpyDeviceToHost) == hipSuccess && (dev[0] != n_cand || dev[1] != n_match))
      fprintf(stderr, "LMX_DEBUG_COLLECT: slot %d host mirror {cand %u, match %u} != device {cand %u, match %u}\n", slot, n_cand, n_match, dev[0], dev[1]);
  }
  c->stat_cands = n_cand; c->stat_matches = n_match;
  if (reinterpret_cast<uint32_t*>(c->h_out)[6] != 0) {
    // a workgroup of a level-0 quantiser gave up waiting for rows of a streamed frame store (StreamWait): the batch ran on incomplete input
    set_error("the input frame never reached the device: a quantiser waited %u us for the host's stores (streamed upload of lmx_match); nothing was matched",
              c->env.stream_timeout_ticks / 100u);
    return LMX_ERR_HIP;
  }
  if (n_cand > c->cap_total || n_match > c->cap_total) {
    set_error("candidate list overflow: %u candidates / %u matches > capacity %u; raise lmx_ctx_desc.max_candidates", n_cand, n_match, c->cap_total);
    return LMX_ERR_OVERFLOW;
  }
  if (n_match > first) {
    // rare: more matches than the first slice.  The records behind it are read from the device slot itself, and when the header poll above
    // saw the sequence word nobody has waited for the slot's event: the word says that k_refine's last workgroup is through, not that the
    // stream's work on the slot has completed for a copy that does not run on that stream.  So wait for the event now, in that case only
    if (seen) LMX_HIP(hipEventSynchronize(c->done[slot]));
    LMX_HIP(hipMemcpy(c->h_out + 64 + first * sizeof(lmx_raw_match_t), d_slot + 64 + first * sizeof(lmx_raw_match_t),
                      (n_match - first) * sizeof(lmx_raw_match_t), hipMemcpyDeviceToHost));
  }
  const clk::time_point t2 = clk::now();
  const lmx_raw_match_t* recs = reinterpret_cast<const lmx_raw_match_t*>(c->h_out + 64);
  std::vector<std::vector<const lmx_raw_match_t*>> per_frame(n_frames);
  for (uint32_t i = 0; i < n_match; ++i) {
    const int f = recs[i].frame;
    if (f >= 0 && f < n_frames) per_frame[f].push_back(&recs[i]);
  }
  const clk::time_point t3 = clk::now();
  fin.resize(n_frames);
  // frames are independent; worth the upload threads only in the explosive regime (threshold 50: 10^5 records per frame, where the two
  // sorts of a frame take tens of milliseconds: DESIGN.md section 8), never at the reference's thresholds
  if (n_match > (1u << 15) && n_frames > 1) {
    if (!c->pool) c->pool.reset(new CopyPool(upload_threads(c) - 1));
    c->pool->parallel_for(n_frames, [&](int f) { finalize_frame(per_frame[f], fin[f]); });
  } else {
    for (int f = 0; f < n_frames; ++f) finalize_frame(per_frame[f], fin[f]);
  }
  if (c->env.match_trace) {
    c->tm_acc[lmx_ctx::TM_WAIT] += std::chrono::duration<double>(t1 - t0).count();
    c->tm_acc[lmx_ctx::TM_FINALIZE] += std::chrono::duration<double>(clk::now() - t1).count();
  }
  if (c->env.collect_trace) {
    auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    size_t n_final = 0;
    for (int f = 0; f < n_frames; ++f) n_final += fin[f].size();
    fprintf(stderr, "lmx collect: %d frames, %u candidates, %u records -> %zu matches | wait %.1f us, fetch beyond first slice %.1f, group %.1f, order + std::sort + std::unique %.1f\n",
            n_frames, n_cand, n_match, n_final, us(t0, t1), us(t1, t2), us(t2, t3), us(t3, clk::now()));
  }
  return LMX_OK;
}

lmx_status lmx_ctx_collect(lmx_ctx* c, int32_t n_frames, lmx_match_t* out, size_t cap, size_t* n_out) {
  return lmx::guarded("lmx_ctx_collect", [&]() -> lmx_status {
  if (!c || !n_out || (cap > 0 && !out)) { set_error("lmx_ctx_collect: null argument"); return LMX_ERR_INVALID_ARG; }
  std::vector<std::vector<HostMatch>> fin;
  lmx_status st = collect_impl(c, n_frames, fin);
  if (st != LMX_OK) { for (int f = 0; f < n_frames; ++f) n_out[f] = 0; return st; }
  for (int f = 0; f < n_frames; ++f) {
    n_out[f] = fin[f].size();
    const size_t n = std::min(cap, fin[f].size());
    for (size_t i = 0; i < n; ++i) out[(size_t)f * cap + i] = fin[f][i].m;
    if (fin[f].size() > cap) { set_error("frame %d: %zu matches > output capacity %zu", f, fin[f].size(), cap); st = LMX_ERR_OVERFLOW; }
  }
  return st;
  });
}

lmx_status lmx_ctx_collect_flat(lmx_ctx* c, int32_t n_frames, lmx_match_t* out, size_t cap_total, size_t* offsets) {
  return lmx::guarded("lmx_ctx_collect_flat", [&]() -> lmx_status {
  if (!c || !offsets || (cap_total > 0 && !out)) { set_error("lmx_ctx_collect_flat: null argument"); return LMX_ERR_INVALID_ARG; }
  std::vector<std::vector<HostMatch>> fin;
  lmx_status st = collect_impl(c, n_frames, fin);
  if (st != LMX_OK) { for (int f = 0; f <= n_frames; ++f) offsets[f] = 0; return st; }
  size_t pos = 0;
  offsets[0] = 0;
  for (int f = 0; f < n_frames; ++f) {
    for (size_t i = 0; i < fin[f].size(); ++i, ++pos)
      if (pos < cap_total) out[pos] = fin[f][i].m;
    offsets[f + 1] = pos;
  }
  if (pos > cap_total) { set_error("%zu matches > output capacity %zu", pos, cap_total); return LMX_ERR_OVERFLOW; }
  return LMX_OK;
  });
}

lmx_status lmx_ctx_set_cluster_sidecar(lmx_ctx* c, const double* obj_origin_dists, const int32_t* rects, size_t n_templates, const lmx_cluster_params* params) {
  if (!c || !obj_origin_dists || !rects || !params || n_templates == 0) { set_error("lmx_ctx_set_cluster_sidecar: invalid argument"); return LMX_ERR_INVALID_ARG; }
  if (params->vote_row_col_step <= 0) { set_error("vote_row_col_step must be positive"); return LMX_ERR_INVALID_ARG; }
  // the reference compares `size() <= thresh` with the int converted to size_t (src/rgbdDetector.cpp:72-85): a negative threshold would drop
  // every cluster there, and its erase-while-iterating is undefined anyway; refused so that the host and device chains cannot diverge
  if (params->cluster_size_thresh < 0) { set_error("cluster_size_thresh must not be negative"); return LMX_ERR_INVALID_ARG; }
  if (lmx_status vs = check_vote_rings(obj_origin_dists, n_templates, params)) return vs;
  LMX_HIP(hipSetDevice(c->device));
  if (sync_lanes(c) != LMX_OK) return LMX_ERR_HIP;   // a kernel may still read the previous side-car
  if (c->d_f2_dists) (void)hipFree(c->d_f2_dists);
  if (c->d_f2_rects) (void)hipFree(c->d_f2_rects);
  c->d_f2_dists = nullptr; c->d_f2_rects = nullptr; c->f2_sidecar = false;
  LMX_HIP(hipMalloc((void**)&c->d_f2_dists, n_templates * sizeof(double)));
  LMX_HIP(hipMalloc((void**)&c->d_f2_rects, n_templates * 4 * sizeof(int32_t)));
  LMX_HIP(hipMemcpy(c->d_f2_dists, obj_origin_dists, n_templates * sizeof(double), hipMemcpyHostToDevice));
  LMX_HIP(hipMemcpy(c->d_f2_rects, rects, n_templates * 4 * sizeof(int32_t), hipMemcpyHostToDevice));
  c->f2_templates = n_templates; c->f2_params = *params; c->f2_sidecar = true;
  c->f2_host_dists.assign(obj_origin_dists, obj_origin_dists + n_templates);
  c->f2_host_rects.assign(rects, rects + n_templates * 4);
  return LMX_OK;
}

// Rewrites the device table of the per-class side-cars from the context's state (the caller has synchronised the lanes and the chain's stream).
static lmx_status upload_class_table(lmx_ctx* c) {
  F2Class tab[F2_CLASSES];
  for (int k = 0; k < F2_CLASSES; ++k) {
    const lmx_ctx::ClassSidecar& s = c->f2_class[k];
    tab[k] = F2Class{s.d_dists, s.d_rects, (uint32_t)s.dists.size(), s.params.vote_row_col_step, s.params.cluster_size_thresh, 0,
                     s.params.renderer_radius_min, s.params.renderer_radius_step};
  }
  if (!c->d_f2_class_table) LMX_HIP(hipMalloc((void**)&c->d_f2_class_table, sizeof(tab)));
  LMX_HIP(hipMemcpy(c->d_f2_class_table, tab, sizeof(tab), hipMemcpyHostToDevice));
  return LMX_OK;
}

lmx_status lmx_ctx_set_cluster_sidecar_class(lmx_ctx* c, int32_t class_index, const double* obj_origin_dists, const int32_t* rects, size_t n_templates,
                                             const lmx_cluster_params* params) {
  return lmx::guarded("lmx_ctx_set_cluster_sidecar_class", [&]() -> lmx_status {
  if (!c) { set_error("lmx_ctx_set_cluster_sidecar_class: invalid argument"); return LMX_ERR_INVALID_ARG; }
  if (class_index < 0 || class_index >= F2_CLASSES) {
    set_error("lmx_ctx_set_cluster_sidecar_class: class_index %d: the device chain takes classes 0 .. %d; lmx_cluster_matches_classes on the host takes any number",
              class_index, F2_CLASSES - 1);
    return LMX_ERR_INVALID_ARG;
  }
  if (n_templates != 0) {
    if (!obj_origin_dists || !rects || !params) { set_error("lmx_ctx_set_cluster_sidecar_class: invalid argument"); return LMX_ERR_INVALID_ARG; }
    if (params->vote_row_col_step <= 0) { set_error("vote_row_col_step must be positive"); return LMX_ERR_INVALID_ARG; }
    if (params->cluster_size_thresh < 0) { set_error("cluster_size_thresh must not be negative"); return LMX_ERR_INVALID_ARG; }   // see lmx_ctx_set_cluster_sidecar
    if (lmx_status vs = check_vote_rings(obj_origin_dists, n_templates, params)) return vs;
  }
  lmx_ctx::ClassSidecar& k = c->f2_class[class_index];
  if (n_templates == 0 && k.dists.empty()) return LMX_OK;   // nothing to remove
  LMX_HIP(hipSetDevice(c->device));
  if (sync_lanes(c) != LMX_OK) return LMX_ERR_HIP;   // a kernel may still read the previous side-car
  if (c->f2_stream) LMX_HIP(hipStreamSynchronize(c->f2_stream));
  // the new arrays first: a failure leaves the class's side-car, and the device table that points to it, as they were
  double* d_dists = nullptr;
  int32_t* d_rects = nullptr;
  if (n_templates != 0) {
    auto fill = [&]() -> lmx_status {
      LMX_HIP(hipMalloc((void**)&d_dists, n_templates * sizeof(double)));
      LMX_HIP(hipMalloc((void**)&d_rects, n_templates * 4 * sizeof(int32_t)));
      LMX_HIP(hipMemcpy(d_dists, obj_origin_dists, n_templates * sizeof(double), hipMemcpyHostToDevice));
      LMX_HIP(hipMemcpy(d_rects, rects, n_templates * 4 * sizeof(int32_t), hipMemcpyHostToDevice));
      return LMX_OK;
    };
    if (lmx_status st = fill()) { (void)hipFree(d_dists); (void)hipFree(d_rects); return st; }
  }
  const lmx_ctx::ClassSidecar before = k;
  k.d_dists = d_dists; k.d_rects = d_rects; k.dists.clear(); k.rects.clear(); k.params = lmx_cluster_params{};
  if (n_templates != 0) {
    k.dists.assign(obj_origin_dists, obj_origin_dists + n_templates);
    k.rects.assign(rects, rects + n_templates * 4);
    k.params = *params;
  }
  if (lmx_status st = upload_class_table(c)) {   // the device table still names the old arrays: keep them
    (void)hipFree(d_dists); (void)hipFree(d_rects);
    k = before;
    return st;
  }
  if (before.d_dists) (void)hipFree(before.d_dists);
  if (before.d_rects) (void)hipFree(before.d_rects);
  return LMX_OK;
  });
}

// What lmx_ctx_collect_clusters_classes adds: the per-class chain instead of the un-classed one; null = the un-classed calls
struct ClassChain {
  const int32_t* class_base;   // with a score only: class c's crops are templates class_base[c] .. class_base[c + 1] of the joined object
  int32_t n_classes;
  int32_t* cluster_class;      // parallel to the caller's clusters
};

// What lmx_ctx_collect_clusters_depth and lmx_ctx_collect_clusters_depth_normal add to lmx_ctx_collect_clusters; null = the unscored call
struct DepthScore {
  lmx_depth_templates* templates;
  int32_t class_index;
  double no_value;
  lmx_depth_diff_t* diffs;   // parallel to the caller's matches; may be null
  bool normal;               // score by lmx_match_value of both terms instead of lmx_depth_value
  lmx_normal_diff_t* ndiffs; // normal only: parallel to the caller's matches; may be null
};

// The refusals every cluster chain shares, collect and export (lmx_ctx_export_clusters_on) alike.  The side-car(s) of the chosen chain:
static lmx_status check_chain_sidecar(const char* what, const lmx_ctx* c, bool classes) {
  if (classes) {
    bool any = false;
    for (const lmx_ctx::ClassSidecar& k : c->f2_class) any = any || !k.dists.empty();
    if (!any) { set_error("%s: call lmx_ctx_set_cluster_sidecar_class first", what); return LMX_ERR_INVALID_ARG; }
  } else if (!c->f2_sidecar) { set_error("%s: call lmx_ctx_set_cluster_sidecar first", what); return LMX_ERR_INVALID_ARG; }
  return LMX_OK;
}

// ... and what a score needs (depth null: nothing): the templates against the context and the side-car(s), the normals, the scene against
// the enqueue of n_frames frames.  The caller holds the templates' mutex.
static lmx_status check_chain_score(const char* what, const lmx_ctx* c, int32_t n_frames, const DepthScore* depth, const ClassChain* cls) {
  if (!depth) return LMX_OK;
  const DepthSceneInfo sc = depth_templates_scene(depth->templates);
  if (sc.device != c->device) { set_error("%s: the templates live on device %d, the context on device %d", what, sc.device, c->device); return LMX_ERR_INVALID_ARG; }
  if (cls) {   // the joined object holds exactly the classes' side-cars, one class after the other
    const int32_t* cb = cls->class_base;
    if (!cb || cls->n_classes < 1 || cls->n_classes > F2_CLASSES) { set_error("%s: class_base must hold n_classes + 1 entries, n_classes 1 .. %d", what, F2_CLASSES); return LMX_ERR_INVALID_ARG; }
    if (cb[0] != 0) { set_error("%s: class_base[0] = %d, not 0", what, cb[0]); return LMX_ERR_INVALID_ARG; }
    for (int k = 0; k < F2_CLASSES; ++k) {
      const size_t have = c->f2_class[k].dists.size();
      if (k >= cls->n_classes) {
        if (have) { set_error("%s: class %d has a side-car of %zu templates but class_base ends at class %d", what, k, have, cls->n_classes - 1); return LMX_ERR_INVALID_ARG; }
      } else if (cb[k + 1] < cb[k] || (size_t)(cb[k + 1] - cb[k]) != have) {
        set_error("%s: class %d: class_base gives it templates %d .. %d but its side-car holds %zu templates", what, k, cb[k], cb[k + 1], have);
        return LMX_ERR_INVALID_ARG;
      }
    }
    if (cb[cls->n_classes] != sc.count) { set_error("%s: class_base ends at %d but the object holds %d depth templates", what, cb[cls->n_classes], sc.count); return LMX_ERR_INVALID_ARG; }
  } else if ((size_t)sc.count != c->f2_templates) { set_error("%s: %d depth templates but the side-car holds %zu templates", what, sc.count, c->f2_templates); return LMX_ERR_INVALID_ARG; }
  if (depth->normal && !sc.normals) { set_error("%s: call lmx_depth_templates_enable_normals first", what); return LMX_ERR_INVALID_ARG; }
  if (sc.n_frames < 1) { set_error("%s: no scene uploaded: call lmx_depth_templates_upload_scene first", what); return LMX_ERR_INVALID_ARG; }
  if (sc.n_frames != n_frames) { set_error("%s: the uploaded scene holds %d frames, the enqueue had %d", what, sc.n_frames, n_frames); return LMX_ERR_INVALID_ARG; }
  if (sc.W != c->desc.width || sc.H != c->desc.height) { set_error("%s: the uploaded scene is %d x %d, the context's frames are %d x %d", what, sc.W, sc.H, c->desc.width, c->desc.height); return LMX_ERR_INVALID_ARG; }
  return LMX_OK;
}

// Room for one result of `elem` bytes per raw record of the slot being collected (and, with elem 1, for the large-frame kernel's workspace).
// Nothing reads the old buffer: every call ends synchronised.
static lmx_status grow_rec_diffs(void** d, size_t* cap, size_t n, size_t elem) {
  if (n <= *cap) return LMX_OK;
  if (*d) (void)hipFree(*d);
  *d = nullptr; *cap = 0;
  const size_t want = std::max<size_t>(n, 4096);
  LMX_HIP(hipMalloc(d, want * elem));
  *cap = want;
  return LMX_OK;
}

// What the chain's kernels take of context slot `slot`, whoever launches them: the slot, the caller's output rows, and the context's
// un-classed side-car (not read by the CLASSES forms, nor with do_clusters 0).  The caller adds its score and class fields.
static F2Params chain_slot_params(const lmx_ctx* c, int slot, int32_t n_frames, lmx_match_t* matches, uint32_t* counts, lmx_cluster_t* clusters, int32_t* members,
                                  uint8_t* scratch, bool do_clusters) {
  F2Params p{};
  p.recs = reinterpret_cast<const lmx_raw_match_t*>(c->d_out_slot[slot] + 64);
  p.hdr = reinterpret_cast<const uint32_t*>(c->d_out_slot[slot]);
  p.cap = c->cap_total; p.n_frames = n_frames;
  p.out_matches = matches; p.out_counts = counts; p.out_clusters = clusters; p.out_members = members; p.scratch = scratch;
  p.dists = c->d_f2_dists; p.rects = c->d_f2_rects; p.n_templates = (uint32_t)c->f2_templates;
  p.step = c->f2_params.vote_row_col_step; p.size_thresh = c->f2_params.cluster_size_thresh; p.do_clusters = do_clusters ? 1 : 0;
  p.radius_min = c->f2_params.renderer_radius_min; p.radius_step = c->f2_params.renderer_radius_step;
  return p;
}

// The body of lmx_ctx_collect_clusters and lmx_ctx_collect_clusters_depth (`what` names the entry point in messages).  With `depth`, the
// caller holds the templates' mutex.
static lmx_status collect_clusters_impl(const char* what, lmx_ctx* c, int32_t n_frames, const DepthScore* depth, const ClassChain* cls, lmx_match_t* matches, size_t cap_matches,
                                        size_t* match_offsets, lmx_cluster_t* clusters, size_t cap_clusters, size_t* cluster_offsets, int32_t* members,
                                        size_t cap_members) {
  if (lmx_status st = check_chain_sidecar(what, c, cls != nullptr)) return st;
  if (c->outstanding < 1) { set_error("%s: nothing enqueued", what); return LMX_ERR_INVALID_ARG; }
  const int slot = (c->head + c->n_slots - c->outstanding) % c->n_slots;  // oldest outstanding enqueue
  if (n_frames != c->slot_frames[slot]) { set_error("%s: n_frames=%d but the enqueue had %d", what, n_frames, c->slot_frames[slot]); return LMX_ERR_INVALID_ARG; }
  if (lmx_status st = check_chain_score(what, c, n_frames, depth, cls)) return st;   // every refusal comes before the enqueue is consumed: it stays outstanding
  LMX_HIP(hipSetDevice(c->device));
  for (int f = 0; f <= n_frames; ++f) match_offsets[f] = cluster_offsets[f] = 0;
  const size_t F = (size_t)c->F;
  const size_t off_counts = F * F2_MAX * sizeof(lmx_match_t), off_clusters = off_counts + ((F * 4 * sizeof(uint32_t) + 63) & ~(size_t)63),
               off_members = off_clusters + F * F2_MAX * sizeof(lmx_cluster_t), out_bytes = off_members + F * F2_MAX * sizeof(int32_t);
  if (!c->h_f2_out) {
    lmx_status st;
    uint8_t* dv = nullptr;
    LMX_HIP(hipHostMalloc((void**)&c->h_f2_out, out_bytes, hipHostMallocMapped));
    LMX_HIP(hipHostGetDevicePointer((void**)&dv, c->h_f2_out, 0));
    std::memset(c->h_f2_out + off_counts, 0, F * 4 * sizeof(uint32_t));
    c->d_f2_matches = reinterpret_cast<lmx_match_t*>(dv); c->d_f2_counts = reinterpret_cast<uint32_t*>(dv + off_counts);
    c->d_f2_clusters = reinterpret_cast<lmx_cluster_t*>(dv + off_clusters); c->d_f2_members = reinterpret_cast<int32_t*>(dv + off_members);
    if ((st = dev_alloc(c, &c->d_f2_scratch, F * F2_MAX * 32, false)) != LMX_OK) return st;
    LMX_HIP(hipStreamCreateWithFlags(&c->f2_stream, hipStreamNonBlocking));
    LMX_HIP(hipStreamSynchronize(c->stream));
  }
  if (cls && !c->h_f2_cluster_class) {
    LMX_HIP(hipHostMalloc((void**)&c->h_f2_cluster_class, F * F2_MAX * sizeof(int32_t), hipHostMallocMapped));
    LMX_HIP(hipHostGetDevicePointer((void**)&c->d_f2_cluster_class, c->h_f2_cluster_class, 0));
  }
  if (cls && depth && (c->f2_class_base.size() != (size_t)cls->n_classes + 1 || !std::equal(c->f2_class_base.begin(), c->f2_class_base.end(), cls->class_base))) {
    // (every earlier call that read the old table ended synchronised)
    if (!c->d_f2_class_base) LMX_HIP(hipMalloc((void**)&c->d_f2_class_base, (F2_CLASSES + 1) * sizeof(int32_t)));
    LMX_HIP(hipMemcpy(c->d_f2_class_base, cls->class_base, ((size_t)cls->n_classes + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    c->f2_class_base.assign(cls->class_base, cls->class_base + cls->n_classes + 1);
  }
  if (depth && !c->h_f2_diffs) {
    LMX_HIP(hipHostMalloc((void**)&c->h_f2_diffs, F * F2_MAX * sizeof(lmx_depth_diff_t), hipHostMallocMapped));
    LMX_HIP(hipHostGetDevicePointer((void**)&c->d_f2_diffs, c->h_f2_diffs, 0));
    if (lmx_status st = dev_alloc(c, &c->d_f2_diff_scratch, F * 2 * F2_MAX, false)) return st;
  }
  if (depth && depth->normal && !c->h_f2_ndiffs) {
    LMX_HIP(hipHostMalloc((void**)&c->h_f2_ndiffs, F * F2_MAX * sizeof(lmx_normal_diff_t), hipHostMallocMapped));
    LMX_HIP(hipHostGetDevicePointer((void**)&c->d_f2_ndiffs, c->h_f2_ndiffs, 0));
    if (lmx_status st = dev_alloc(c, &c->d_f2_ndiff_scratch, F * 2 * F2_MAX, false)) return st;
  }
  LMX_HIP(hipEventSynchronize(c->done[slot]));
  if (lmx_status xs = wait_exports(c, slot)) return xs;   // an export may still read the slot this call frees
  c->outstanding -= 1;
  if (c->outstanding == 0) drain_profiling(c);
  const uint32_t* h_hdr = reinterpret_cast<const uint32_t*>(c->h_out_slot[slot]);
  const uint32_t n_cand = h_hdr[0], n_match = h_hdr[1];
  c->stat_cands = n_cand; c->stat_matches = n_match;
  if (n_cand > c->cap_total || n_match > c->cap_total) {
    set_error("candidate list overflow: %u candidates / %u matches > capacity %u; raise lmx_ctx_desc.max_candidates", n_cand, n_match, c->cap_total);
    return LMX_ERR_OVERFLOW;
  }
  // on its own stream: the slot's kernels have finished (its event was waited for above), and the lane's stream may already carry later
  // batches that this collect must not wait for
  hipStream_t s = c->f2_stream;
  const F2Score score = f2_score(depth != nullptr, depth && depth->normal);
  F2Params p = chain_slot_params(c, slot, n_frames, c->d_f2_matches, c->d_f2_counts, c->d_f2_clusters, c->d_f2_members, c->d_f2_scratch, true);
  if (cls) { p.classes = c->d_f2_class_table; p.out_cluster_class = c->d_f2_cluster_class; }
  if (depth) {
    if (lmx_status st = grow_rec_diffs((void**)&c->d_f2_rec_diffs, &c->f2_rec_diffs_cap, n_match, sizeof(lmx_depth_diff_t))) return st;
    if (depth->normal)
      if (lmx_status st = grow_rec_diffs((void**)&c->d_f2_rec_ndiffs, &c->f2_rec_ndiffs_cap, n_match, sizeof(lmx_normal_diff_t))) return st;
    // the scene's copies, one workgroup per raw record (the count is the header's, read above), the scored chain: one synchronisation
    DepthWalk w;
    w.recs = p.recs; w.n = n_match; w.class_index = depth->class_index;
    if (cls) { w.d_class_base = c->d_f2_class_base; w.n_classes = cls->n_classes; }
    w.d_diffs = c->d_f2_rec_diffs; w.d_ndiffs = depth->normal ? c->d_f2_rec_ndiffs : nullptr;
    if (lmx_status st = depth_launch_walk(depth->templates, s, w)) return st;
    p.diffs = c->d_f2_rec_diffs; p.out_diffs = c->d_f2_diffs; p.diff_scratch = c->d_f2_diff_scratch; p.no_value = depth->no_value;
    if (depth->normal) { p.ndiffs = c->d_f2_rec_ndiffs; p.out_ndiffs = c->d_f2_ndiffs; p.ndiff_scratch = c->d_f2_ndiff_scratch; }
  }
  launch_f2(s, p, score, cls != nullptr);
  LMX_HIP(hipGetLastError());
  LMX_HIP(hipStreamSynchronize(s));
  const uint32_t* counts = reinterpret_cast<const uint32_t*>(c->h_f2_out + off_counts);
  const lmx_match_t* all_m = reinterpret_cast<const lmx_match_t*>(c->h_f2_out);
  const lmx_cluster_t* all_c = reinterpret_cast<const lmx_cluster_t*>(c->h_f2_out + off_clusters);
  const int32_t* all_mem = reinterpret_cast<const int32_t*>(c->h_f2_out + off_members);
  // frames the LDS kernel handed back for their record count and the large-frame kernel takes: a second launch on exactly those, one
  // workgroup each, on workspace parts allocated for as many (a call without such a frame launches nothing and allocates nothing)
  std::vector<int32_t> large;
  std::vector<int> large_part(n_frames, -1);
  std::vector<uint32_t> lcounts;
  F2LargeLayout lay{};
  if (c->env.f2_large)
    for (int f = 0; f < n_frames; ++f)
      if (counts[(size_t)f * 4 + 3] == 1 && counts[(size_t)f * 4] <= (uint32_t)F2_LARGE_MAX) { large_part[f] = (int)large.size(); large.push_back(f); }
  if (!large.empty()) {
    lay = f2_large_layout(score);
    if (lmx_status gs = grow_rec_diffs((void**)&c->d_f2l_ws, &c->f2l_ws_bytes, large.size() * (size_t)lay.bytes, 1)) return gs;
    if (!c->d_f2l_frames) LMX_HIP(hipMalloc((void**)&c->d_f2l_frames, F * sizeof(int32_t)));
    if (!c->d_f2l_counts) LMX_HIP(hipMalloc((void**)&c->d_f2l_counts, F * 4 * sizeof(uint32_t)));
    LMX_HIP(hipMemcpy(c->d_f2l_frames, large.data(), large.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    F2LargeParams lp{p, c->d_f2l_frames, c->d_f2l_ws, lay};
    lp.p.out_counts = c->d_f2l_counts;
    launch_f2_large(s, lp, (int)large.size(), score, cls != nullptr);
    LMX_HIP(hipGetLastError());
    LMX_HIP(hipStreamSynchronize(s));
    lcounts.resize(large.size() * 4);
    LMX_HIP(hipMemcpy(lcounts.data(), c->d_f2l_counts, lcounts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  // where each frame's result lies: 0 the LDS kernel's pinned rows, 1 the large kernel's workspace part, 2 nowhere yet (the host path)
  std::vector<int> where(n_frames, 0);
  lmx_chain_stats cs{};
  cs.frames = n_frames;
  for (int f = 0; f < n_frames; ++f) {
    const uint32_t status = counts[(size_t)f * 4 + 3];
    if (status == 1) cs.max_frame_records = std::max<int32_t>(cs.max_frame_records, (int32_t)std::min<uint32_t>(counts[(size_t)f * 4], 0x7fffffffu));
    if (status == 0) { cs.frames_lds += 1; continue; }
    if (large_part[f] >= 0 && lcounts[(size_t)large_part[f] * 4 + 3] == 0) { where[f] = 1; cs.frames_large += 1; continue; }
    where[f] = 2;
    if (status == 1 && large_part[f] < 0) cs.frames_host_records += 1;
    else cs.frames_host_other += 1;
  }
  cs.large_workspace_bytes = (int64_t)c->f2l_ws_bytes;
  c->chain_stats = cs;
  // frames no kernel could take (too many records, rings outside the packed range): the host path on the slot's records
  std::vector<lmx_raw_match_t> host_recs;
  const bool any_host = cs.frames_host_records + cs.frames_host_other > 0;
  if (any_host) {
    host_recs.resize(n_match);
    if (n_match) LMX_HIP(hipMemcpy(host_recs.data(), c->d_out_slot[slot] + 64, (size_t)n_match * sizeof(lmx_raw_match_t), hipMemcpyDeviceToHost));
  }
  lmx_status st = LMX_OK;
  size_t mpos = 0, cpos = 0, mempos = 0;
  std::vector<HostMatch> fin;
  std::vector<lmx_match_t> fm;
  std::vector<lmx_cluster_t> fc;
  std::vector<int32_t> fmem;
  std::vector<lmx_depth_diff_t> fd;
  std::vector<lmx_normal_diff_t> fn;
  std::vector<double> fv;
  std::vector<int32_t> fcls;
  std::vector<lmx_class_sidecar> host_classes;
  if (cls && any_host)
    for (const lmx_ctx::ClassSidecar& k : c->f2_class) host_classes.push_back(lmx_class_sidecar{k.dists.data(), k.rects.data(), k.dists.size(), k.params});
  for (int f = 0; f < n_frames; ++f) {
    size_t nm = 0, nc = 0, nmem = 0;
    if (where[f] == 1) {   // the large kernel's part of the workspace: read back what its counts say
      const uint32_t* lc = lcounts.data() + (size_t)large_part[f] * 4;
      const uint8_t* part = c->d_f2l_ws + (size_t)large_part[f] * lay.bytes;
      nm = lc[0]; nc = lc[1]; nmem = lc[2];
      fm.resize(cap_matches ? nm : 0); fc.resize(nc); fmem.resize(nmem);
      if (cap_matches && nm) {
        LMX_HIP(hipMemcpy(fm.data(), part + lay.matches, nm * sizeof(lmx_match_t), hipMemcpyDeviceToHost));
        if (depth && depth->diffs) { fd.resize(nm); LMX_HIP(hipMemcpy(fd.data(), part + lay.diffs, nm * sizeof(lmx_depth_diff_t), hipMemcpyDeviceToHost)); }
        if (depth && depth->ndiffs) { fn.resize(nm); LMX_HIP(hipMemcpy(fn.data(), part + lay.ndiffs, nm * sizeof(lmx_normal_diff_t), hipMemcpyDeviceToHost)); }
      }
      if (nc) LMX_HIP(hipMemcpy(fc.data(), part + lay.clusters, nc * sizeof(lmx_cluster_t), hipMemcpyDeviceToHost));
      if (nmem) LMX_HIP(hipMemcpy(fmem.data(), part + lay.members, nmem * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (cls) { fcls.resize(nc); if (nc) LMX_HIP(hipMemcpy(fcls.data(), part + lay.cluster_class, nc * sizeof(int32_t), hipMemcpyDeviceToHost)); }
    } else if (where[f] == 0) {
      nm = counts[(size_t)f * 4 + 0]; nc = counts[(size_t)f * 4 + 1]; nmem = counts[(size_t)f * 4 + 2];
      if (cap_matches) fm.assign(all_m + (size_t)F2_MAX * f, all_m + (size_t)F2_MAX * f + nm);
      else fm.clear();
      if (depth && depth->diffs && cap_matches) fd.assign(c->h_f2_diffs + (size_t)F2_MAX * f, c->h_f2_diffs + (size_t)F2_MAX * f + nm);
      if (depth && depth->ndiffs && cap_matches) fn.assign(c->h_f2_ndiffs + (size_t)F2_MAX * f, c->h_f2_ndiffs + (size_t)F2_MAX * f + nm);
      fc.assign(all_c + (size_t)F2_MAX * f, all_c + (size_t)F2_MAX * f + nc);
      fmem.assign(all_mem + (size_t)F2_MAX * f, all_mem + (size_t)F2_MAX * f + nmem);
      if (cls) fcls.assign(c->h_f2_cluster_class + (size_t)F2_MAX * f, c->h_f2_cluster_class + (size_t)F2_MAX * f + nc);
    } else {
      std::vector<const lmx_raw_match_t*> recs;
      for (const lmx_raw_match_t& r : host_recs)
        if (r.frame == f) recs.push_back(&r);
      finalize_frame(recs, fin);
      nm = fin.size();
      fm.resize(nm);
      for (size_t i = 0; i < nm; ++i) fm[i] = fin[i].m;
      fc.resize(std::max<size_t>(nm, 1)); fmem.resize(std::max<size_t>(nm, 1));
      if (cls) fcls.resize(std::max<size_t>(nm, 1));
      size_t got = 0;
      lmx_status hs;
      if (depth) {   // the final matches against the resident scene (the job form of k_walk), then the host chain on their values
        fd.resize(std::max<size_t>(nm, 1)); fv.resize(std::max<size_t>(nm, 1));
        if (depth->normal) fn.resize(std::max<size_t>(nm, 1));
        hs = cls ? depth_diff_resident_classes(depth->templates, fm.data(), nm, f, cls->class_base, cls->n_classes, fd.data(), depth->normal ? fn.data() : nullptr)
                 : depth_diff_resident(depth->templates, fm.data(), nm, f, depth->class_index, fd.data(), depth->normal ? fn.data() : nullptr);
        if (hs != LMX_OK) return hs;
        for (size_t i = 0; i < nm; ++i) fv[i] = depth->normal ? nv::value(fd[i], fn[i], depth->no_value) : dv::value(fd[i], depth->no_value);
        if (cls) hs = lmx_cluster_matches_classes(fm.data(), nm, fv.data(), host_classes.data(), F2_CLASSES, fc.data(), fcls.data(), fc.size(), &got, fmem.data(), fmem.size());
        else hs = lmx_cluster_matches_scored(fm.data(), nm, fv.data(), c->f2_host_dists.data(), c->f2_host_rects.data(), c->f2_templates, &c->f2_params, fc.data(),
                                        fc.size(), &got, fmem.data(), fmem.size());
      } else if (cls) {
        hs = lmx_cluster_matches_classes(fm.data(), nm, nullptr, host_classes.data(), F2_CLASSES, fc.data(), fcls.data(), fc.size(), &got, fmem.data(), fmem.size());
      } else {
        hs = lmx_cluster_matches(fm.data(), nm, c->f2_host_dists.data(), c->f2_host_rects.data(), c->f2_templates, &c->f2_params, fc.data(), fc.size(), &got,
                                 fmem.data(), fmem.size());
      }
      if (hs != LMX_OK) return hs;
      nc = got; nmem = 0;
      for (size_t i = 0; i < nc; ++i) nmem += (size_t)fc[i].member_count;
    }
    if (cap_matches) {
      if (mpos + nm > cap_matches) st = LMX_ERR_OVERFLOW;
      else if (nm) {
        std::memcpy(matches + mpos, fm.data(), nm * sizeof(lmx_match_t));   // (an empty vector's data() may be null)
        if (depth && depth->diffs) std::memcpy(depth->diffs + mpos, fd.data(), nm * sizeof(lmx_depth_diff_t));
        if (depth && depth->ndiffs) std::memcpy(depth->ndiffs + mpos, fn.data(), nm * sizeof(lmx_normal_diff_t));
      }
    }
    if (cpos + nc <= cap_clusters && mempos + nmem <= cap_members) {
      for (size_t i = 0; i < nc; ++i) { clusters[cpos + i] = fc[i]; clusters[cpos + i].member_begin += (int32_t)mempos; }
      if (nmem) std::memcpy(members + mempos, fmem.data(), nmem * sizeof(int32_t));
      if (cls && nc) std::memcpy(cls->cluster_class + cpos, fcls.data(), nc * sizeof(int32_t));
    } else {
      st = LMX_ERR_OVERFLOW;
    }
    mpos += nm; cpos += nc; mempos += nmem;
    match_offsets[f + 1] = mpos; cluster_offsets[f + 1] = cpos;
  }
  if (st != LMX_OK) set_error("%zu matches / %zu clusters / %zu members exceed the output capacity", mpos, cpos, mempos);
  return st;
}

lmx_status lmx_ctx_collect_clusters(lmx_ctx* c, int32_t n_frames, lmx_match_t* matches, size_t cap_matches, size_t* match_offsets, lmx_cluster_t* clusters,
                                    size_t cap_clusters, size_t* cluster_offsets, int32_t* members, size_t cap_members) {
  return lmx::guarded("lmx_ctx_collect_clusters", [&]() -> lmx_status {
  if (!c || !match_offsets || !cluster_offsets || (cap_matches > 0 && !matches) || (cap_clusters > 0 && !clusters) || (cap_members > 0 && !members)) {
    set_error("lmx_ctx_collect_clusters: null argument");
    return LMX_ERR_INVALID_ARG;
  }
  return collect_clusters_impl("lmx_ctx_collect_clusters", c, n_frames, nullptr, nullptr, matches, cap_matches, match_offsets, clusters, cap_clusters, cluster_offsets,
                               members, cap_members);
  });
}

lmx_status lmx_ctx_collect_clusters_depth(lmx_ctx* c, int32_t n_frames, lmx_depth_templates* templates, int32_t class_index, double no_value,
                                          lmx_match_t* matches, size_t cap_matches, size_t* match_offsets, lmx_depth_diff_t* diffs, lmx_cluster_t* clusters,
                                          size_t cap_clusters, size_t* cluster_offsets, int32_t* members, size_t cap_members) {
  return lmx::guarded("lmx_ctx_collect_clusters_depth", [&]() -> lmx_status {
  if (no_value != no_value) { set_error("lmx_ctx_collect_clusters_depth: no_value is not a number (the score order would be undefined)"); return LMX_ERR_INVALID_ARG; }
  if (!c || !templates || !match_offsets || !cluster_offsets || (cap_matches > 0 && !matches) || (cap_clusters > 0 && !clusters) || (cap_members > 0 && !members)) {
    set_error("lmx_ctx_collect_clusters_depth: null argument");
    return LMX_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lk(depth_templates_mutex(templates));   // held for the whole call: the scene and the object's buffers stay put
  const DepthScore depth{templates, class_index, no_value, diffs, false, nullptr};
  return collect_clusters_impl("lmx_ctx_collect_clusters_depth", c, n_frames, &depth, nullptr, matches, cap_matches, match_offsets, clusters, cap_clusters,
                               cluster_offsets, members, cap_members);
  });
}

lmx_status lmx_ctx_collect_clusters_depth_normal(lmx_ctx* c, int32_t n_frames, lmx_depth_templates* templates, int32_t class_index, double no_value,
                                                 lmx_match_t* matches, size_t cap_matches, size_t* match_offsets, lmx_depth_diff_t* diffs,
                                                 lmx_normal_diff_t* ndiffs, lmx_cluster_t* clusters, size_t cap_clusters, size_t* cluster_offsets,
                                                 int32_t* members, size_t cap_members) {
  return lmx::guarded("lmx_ctx_collect_clusters_depth_normal", [&]() -> lmx_status {
  if (no_value != no_value) { set_error("lmx_ctx_collect_clusters_depth_normal: no_value is not a number (the score order would be undefined)"); return LMX_ERR_INVALID_ARG; }
  if (!c || !templates || !match_offsets || !cluster_offsets || (cap_matches > 0 && !matches) || (cap_clusters > 0 && !clusters) || (cap_members > 0 && !members)) {
    set_error("lmx_ctx_collect_clusters_depth_normal: null argument");
    return LMX_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lk(depth_templates_mutex(templates));   // held for the whole call: the scene and the object's buffers stay put
  const DepthScore depth{templates, class_index, no_value, diffs, true, ndiffs};
  return collect_clusters_impl("lmx_ctx_collect_clusters_depth_normal", c, n_frames, &depth, nullptr, matches, cap_matches, match_offsets, clusters, cap_clusters,
                               cluster_offsets, members, cap_members);
  });
}

lmx_status lmx_ctx_collect_clusters_classes(lmx_ctx* c, int32_t n_frames, const lmx_class_score* score, lmx_match_t* matches, size_t cap_matches,
                                            size_t* match_offsets, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs, lmx_cluster_t* clusters,
                                            int32_t* cluster_class, size_t cap_clusters, size_t* cluster_offsets, int32_t* members, size_t cap_members) {
  return lmx::guarded("lmx_ctx_collect_clusters_classes", [&]() -> lmx_status {
  const char* const what = "lmx_ctx_collect_clusters_classes";
  if (!c || !match_offsets || !cluster_offsets || (cap_matches > 0 && !matches) || (cap_clusters > 0 && (!clusters || !cluster_class)) ||
      (cap_members > 0 && !members) || (score && !score->templates)) {
    set_error("%s: null argument", what);
    return LMX_ERR_INVALID_ARG;
  }
  if (!score) {
    const ClassChain cls{nullptr, 0, cluster_class};
    return collect_clusters_impl(what, c, n_frames, nullptr, &cls, matches, cap_matches, match_offsets, clusters, cap_clusters, cluster_offsets, members, cap_members);
  }
  if (score->no_value != score->no_value) { set_error("%s: no_value is not a number (the score order would be undefined)", what); return LMX_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(depth_templates_mutex(score->templates));   // held for the whole call: the scene and the object's buffers stay put
  const DepthScore depth{score->templates, -1, score->no_value, diffs, score->normals != 0, score->normals ? ndiffs : nullptr};
  const ClassChain cls{score->class_base, score->n_classes, cluster_class};
  return collect_clusters_impl(what, c, n_frames, &depth, &cls, matches, cap_matches, match_offsets, clusters, cap_clusters, cluster_offsets, members, cap_members);
  });
}

lmx_status lmx_ctx_chain_stats(lmx_ctx* c, lmx_chain_stats* out) {
  if (!c || !out) { set_error("lmx_ctx_chain_stats: null argument"); return LMX_ERR_INVALID_ARG; }
  *out = c->chain_stats;
  return LMX_OK;
}

lmx_status lmx_ctx_raw_matches(lmx_ctx* c, void** d_records, void** d_counts, size_t* capacity) {
  if (!c) { set_error("lmx_ctx_raw_matches: null context"); return LMX_ERR_INVALID_ARG; }
  if (d_records) *d_records = c->d_records();
  if (d_counts) *d_counts = c->d_out;  // uint32[16] header: [0] = candidates, [1] = matches
  if (capacity) *capacity = c->cap_total;
  return LMX_OK;
}

lmx_status lmx_ctx_export_raw_on(lmx_ctx* c, void* d_block, size_t capacity_records, void* stream) {
  if (!c || !d_block) { set_error("lmx_ctx_export_raw: null argument"); return LMX_ERR_INVALID_ARG; }
  LMX_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const size_t n = std::min<size_t>(capacity_records, c->cap_total);
  // d_out already has the gather-block layout: [64-byte header][records].  The copy is ordered behind the enqueue that
  // produced the records, whichever lane it ran on
  LMX_HIP(hipStreamWaitEvent(s, c->done[c->last_slot], 0));
  // header + as many records as it counts (<= n), by kernel (see k_publish_records); the rest of the block is don't-care
  launch_publish_records(s, d_block, c->d_out, (uint32_t)n, c->cap_total);
  LMX_HIP(hipGetLastError());
  return LMX_OK;
}

lmx_status lmx_ctx_export_oldest_on(lmx_ctx* c, void* d_block, size_t capacity_records, void* stream) {
  if (!c || !d_block) { set_error("lmx_ctx_export_oldest_on: null argument"); return LMX_ERR_INVALID_ARG; }
  if (c->outstanding < 1) { set_error("lmx_ctx_export_oldest_on: nothing enqueued"); return LMX_ERR_INVALID_ARG; }
  LMX_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const int slot = (c->head + c->n_slots - c->outstanding) % c->n_slots;
  LMX_HIP(hipStreamWaitEvent(s, c->done[slot], 0));
  launch_publish_records(s, d_block, c->d_out_slot[slot], (uint32_t)std::min<size_t>(capacity_records, c->cap_total), c->cap_total);
  LMX_HIP(hipGetLastError());
  return LMX_OK;
}

// One output of an export: plain device memory of the context's device, aligned to its element.
static lmx_status check_export_output(const char* what, const lmx_ctx* c, const char* name, const void* p, size_t align) {
  if ((uintptr_t)p & (align - 1)) { set_error("%s: %s must be aligned to %zu bytes", what, name, align); return LMX_ERR_INVALID_ARG; }
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {   // memory the runtime has never seen
    (void)hipGetLastError();
    set_error("%s: %s is not device memory", what, name);
    return LMX_ERR_INVALID_ARG;
  }
  if (attr.type != hipMemoryTypeDevice || attr.device != c->device) {
    set_error("%s: %s is %s; the outputs are plain device memory of device %d", what, name,
              attr.type == hipMemoryTypeDevice ? "memory of another device" : "pageable, pinned, managed or other host memory", c->device);
    return LMX_ERR_INVALID_ARG;
  }
  return LMX_OK;
}

// What lmx_ctx_export_matches_on and lmx_ctx_export_clusters_on ask of export_impl: the fields of their structs.
struct ExportRequest {
  int32_t oldest, max_large_frames;
  bool clusters, classes;
  F2Score score;
  lmx_depth_templates* templates;  // with a score
  int32_t class_index;
  const int32_t* class_base;
  int32_t n_classes;
  double no_value;
  uint32_t* header;
  int32_t* frame_info;
  lmx_match_t* matches; size_t cap_matches;
  lmx_depth_diff_t* diffs;
  lmx_normal_diff_t* ndiffs;
  lmx_cluster_t* clusters_out; size_t cap_clusters;
  int32_t* cluster_class;
  int32_t* members; size_t cap_members;
};

// The body of both exports (include/lmx.h; kernels: lmx_export.hip, and for a score the device-count walk of lmx_verify.hip).  Every refusal
// comes before anything is queued; nothing below waits on the host for the device except an allocation's first use.
static lmx_status export_impl(const char* what, lmx_ctx* c, int32_t n_frames, const ExportRequest& q, void* stream) {
  if (!c->sets[0].h_stage) { set_error("%s: this context is a member of a device group", what); return LMX_ERR_INVALID_ARG; }
  if (c->outstanding < 1) { set_error("%s: nothing enqueued", what); return LMX_ERR_INVALID_ARG; }
  const int slot = q.oldest ? (c->head + c->n_slots - c->outstanding) % c->n_slots : (c->head + c->n_slots - 1) % c->n_slots;
  if (n_frames != c->slot_frames[slot]) { set_error("%s: n_frames=%d but the enqueue had %d", what, n_frames, c->slot_frames[slot]); return LMX_ERR_INVALID_ARG; }
  if (!q.header || !q.frame_info || !q.matches) { set_error("%s: header, frame_info and matches must not be null", what); return LMX_ERR_INVALID_ARG; }
  const bool clusters = q.clusters, scored = q.score != F2_SIMILARITY, normal = q.score == F2_DEPTH_NORMAL;
  if (clusters)
    if (lmx_status st = check_chain_sidecar(what, c, q.classes)) return st;
  if (clusters && (!q.clusters_out || !q.members)) { set_error("%s: clusters: clusters_out and members must not be null", what); return LMX_ERR_INVALID_ARG; }
  if (q.classes && !q.cluster_class) { set_error("%s: classes: cluster_class must not be null", what); return LMX_ERR_INVALID_ARG; }
  if (scored && (!q.templates || !q.diffs)) { set_error("%s: score %d: templates and diffs must not be null", what, (int)q.score); return LMX_ERR_INVALID_ARG; }
  if (normal && !q.ndiffs) { set_error("%s: score 2: ndiffs must not be null", what); return LMX_ERR_INVALID_ARG; }
  if (scored && q.no_value != q.no_value) { set_error("%s: no_value is not a number (the score order would be undefined)", what); return LMX_ERR_INVALID_ARG; }
  if (q.max_large_frames < 0) { set_error("%s: max_large_frames %d is negative", what, q.max_large_frames); return LMX_ERR_INVALID_ARG; }
  std::unique_lock<std::mutex> lk;   // held during the call: the scene and the object's buffers stay put until the walk is queued
  if (scored) {
    lk = std::unique_lock<std::mutex>(depth_templates_mutex(q.templates));
    const DepthScore depth{q.templates, q.class_index, q.no_value, nullptr, normal, nullptr};
    const ClassChain cls{q.class_base, q.n_classes, nullptr};
    if (lmx_status st = check_chain_score(what, c, n_frames, &depth, q.classes ? &cls : nullptr)) return st;
  }
  LMX_HIP(hipSetDevice(c->device));
  hipStream_t user = static_cast<hipStream_t>(stream);
  if (lmx_status st = check_user_stream(what, user)) return st;
  if (lmx_status st = check_export_output(what, c, "header", q.header, 4)) return st;
  if (lmx_status st = check_export_output(what, c, "frame_info", q.frame_info, 4)) return st;
  if (lmx_status st = check_export_output(what, c, "matches", q.matches, 4)) return st;
  if (clusters) {
    if (lmx_status st = check_export_output(what, c, "clusters_out", q.clusters_out, 8)) return st;
    if (lmx_status st = check_export_output(what, c, "members", q.members, 4)) return st;
  }
  if (scored)
    if (lmx_status st = check_export_output(what, c, "diffs", q.diffs, 8)) return st;
  if (normal)
    if (lmx_status st = check_export_output(what, c, "ndiffs", q.ndiffs, 8)) return st;
  if (q.classes)
    if (lmx_status st = check_export_output(what, c, "cluster_class", q.cluster_class, 4)) return st;
  // the export's own buffers, on first use
  const size_t F = (size_t)c->F;
  const F2LargeLayout lay = f2_large_layout(q.score);
  if (!c->d_xp_rows) {
    const size_t off_clusters = F * F2_MAX * sizeof(lmx_match_t), off_members = off_clusters + F * F2_MAX * sizeof(lmx_cluster_t),
                 off_counts = off_members + F * F2_MAX * sizeof(int32_t), off_list = off_counts + F * 4 * sizeof(uint32_t),
                 off_listed = off_list + F * sizeof(int32_t), off_lcounts = (off_listed + sizeof(uint32_t) + 15) & ~(size_t)15,
                 bytes = off_lcounts + F * 4 * sizeof(uint32_t);
    static_assert((F2_MAX * sizeof(lmx_match_t)) % 16 == 0 && (F2_MAX * sizeof(lmx_cluster_t)) % 16 == 0, "the rows stay 16-byte aligned");
    uint8_t* rows = nullptr;
    lmx_status st;
    if ((st = dev_alloc(c, &rows, bytes, false)) != LMX_OK) return st;
    if ((st = dev_alloc(c, &c->d_xp_scratch, F * F2_MAX * 32, false)) != LMX_OK) return st;
    LMX_HIP(hipStreamCreateWithFlags(&c->export_stream, hipStreamNonBlocking));
    LMX_HIP(hipEventCreateWithFlags(&c->export_dst_ready, hipEventDisableTiming));
    for (int i = 0; i < lmx_ctx::kSlots; ++i) LMX_HIP(hipEventCreateWithFlags(&c->export_done[i], hipEventDisableTiming));
    c->d_xp_matches = reinterpret_cast<lmx_match_t*>(rows); c->d_xp_clusters = reinterpret_cast<lmx_cluster_t*>(rows + off_clusters);
    c->d_xp_members = reinterpret_cast<int32_t*>(rows + off_members); c->d_xp_counts = reinterpret_cast<uint32_t*>(rows + off_counts);
    c->d_xp_large_frames = reinterpret_cast<int32_t*>(rows + off_list); c->d_xp_large_listed = reinterpret_cast<uint32_t*>(rows + off_listed);
    c->d_xp_large_counts = reinterpret_cast<uint32_t*>(rows + off_lcounts);
    c->d_xp_rows = rows;
  }
  // the scored forms' rows, plain device memory (the collect's are mapped pinned memory), and one result per record the slot can hold:
  // the count is not known here
  if (scored && !c->d_xp_diffs) {
    lmx_status st;
    if ((st = dev_alloc(c, &c->d_xp_rec_diffs, (size_t)c->cap_total, false)) != LMX_OK) return st;
    if ((st = dev_alloc(c, &c->d_xp_diff_scratch, F * 2 * F2_MAX, false)) != LMX_OK) return st;
    if ((st = dev_alloc(c, &c->d_xp_diffs, F * F2_MAX, false)) != LMX_OK) return st;
  }
  if (normal && !c->d_xp_ndiffs) {
    lmx_status st;
    if ((st = dev_alloc(c, &c->d_xp_rec_ndiffs, (size_t)c->cap_total, false)) != LMX_OK) return st;
    if ((st = dev_alloc(c, &c->d_xp_ndiff_scratch, F * 2 * F2_MAX, false)) != LMX_OK) return st;
    if ((st = dev_alloc(c, &c->d_xp_ndiffs, F * F2_MAX, false)) != LMX_OK) return st;
  }
  if (q.classes && !c->d_xp_cluster_class)
    if (lmx_status st = dev_alloc(c, &c->d_xp_cluster_class, F * F2_MAX, false)) return st;
  if (q.classes && scored && (c->xp_class_base.size() != (size_t)q.n_classes + 1 || !std::equal(c->xp_class_base.begin(), c->xp_class_base.end(), q.class_base))) {
    if (!c->d_xp_class_base) {
      if (lmx_status st = dev_alloc(c, &c->d_xp_class_base, (size_t)F2_CLASSES + 1, false)) return st;
    }
    LMX_HIP(hipStreamSynchronize(c->export_stream));   // an earlier export's walk may still read the old table
    LMX_HIP(hipMemcpy(c->d_xp_class_base, q.class_base, ((size_t)q.n_classes + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    c->xp_class_base.assign(q.class_base, q.class_base + q.n_classes + 1);
  }
  const int max_large = std::min<int>(q.max_large_frames, n_frames);
  if ((size_t)max_large * lay.bytes > c->xp_large_bytes) {   // an earlier export may still work on the old workspace
    LMX_HIP(hipStreamSynchronize(c->export_stream));
    if (c->d_xp_large_ws) (void)hipFree(c->d_xp_large_ws);
    c->d_xp_large_ws = nullptr; c->xp_large_bytes = 0;
    LMX_HIP(hipMalloc((void**)&c->d_xp_large_ws, (size_t)max_large * lay.bytes));
    c->xp_large_bytes = (size_t)max_large * lay.bytes;
  }
  hipStream_t s = c->export_stream;
  // behind the enqueue that fills the slot, and behind what the caller's stream still does with the outputs
  LMX_HIP(hipStreamWaitEvent(s, c->done[slot], 0));
  LMX_HIP(hipEventRecord(c->export_dst_ready, user));
  LMX_HIP(hipStreamWaitEvent(s, c->export_dst_ready, 0));
  F2Params p = chain_slot_params(c, slot, n_frames, c->d_xp_matches, c->d_xp_counts, c->d_xp_clusters, c->d_xp_members, c->d_xp_scratch, clusters);
  if (q.classes) { p.classes = c->d_f2_class_table; p.out_cluster_class = c->d_xp_cluster_class; }
  if (scored) {
    // the scene's copies, the walk over however many records the slot's header counts, then the scored chain on its results
    DepthWalk w;
    w.recs = p.recs; w.hdr = p.hdr; w.cap = p.cap; w.class_index = q.class_index;
    if (q.classes) { w.d_class_base = c->d_xp_class_base; w.n_classes = q.n_classes; }
    w.d_diffs = c->d_xp_rec_diffs; w.d_ndiffs = normal ? c->d_xp_rec_ndiffs : nullptr;
    if (lmx_status st = depth_launch_walk(q.templates, s, w)) return st;
    lk.unlock();
    p.diffs = c->d_xp_rec_diffs; p.out_diffs = c->d_xp_diffs; p.diff_scratch = c->d_xp_diff_scratch; p.no_value = q.no_value;
    if (normal) { p.ndiffs = c->d_xp_rec_ndiffs; p.out_ndiffs = c->d_xp_ndiffs; p.ndiff_scratch = c->d_xp_ndiff_scratch; }
  }
  launch_f2(s, p, q.score, q.classes);
  ExportParams e{};
  e.recs = p.recs; e.hdr = p.hdr; e.cap = p.cap; e.n_frames = n_frames; e.max_large = max_large;
  e.rows_matches = c->d_xp_matches; e.rows_clusters = c->d_xp_clusters; e.rows_members = c->d_xp_members; e.counts = c->d_xp_counts;
  e.large_ws = c->d_xp_large_ws; e.large_counts = c->d_xp_large_counts; e.lay = lay;
  e.large_frames = c->d_xp_large_frames; e.large_listed = c->d_xp_large_listed;
  e.header = q.header; e.frame_info = q.frame_info; e.matches = q.matches; e.cap_matches = q.cap_matches;
  e.clusters = clusters ? q.clusters_out : nullptr; e.cap_clusters = clusters ? q.cap_clusters : 0;
  e.members = clusters ? q.members : nullptr; e.cap_members = clusters ? q.cap_members : 0;
  if (scored) { e.rows_diffs = c->d_xp_diffs; e.diffs = q.diffs; }
  if (normal) { e.rows_ndiffs = c->d_xp_ndiffs; e.ndiffs = q.ndiffs; }
  if (q.classes) { e.rows_cluster_class = c->d_xp_cluster_class; e.cluster_class = q.cluster_class; }
  if (max_large > 0) {
    launch_export_plan(s, e);
    F2LargeParams lp{p, c->d_xp_large_frames, c->d_xp_large_ws, lay, c->d_xp_large_listed};
    lp.p.out_counts = c->d_xp_large_counts;
    launch_f2_large(s, lp, max_large, q.score, q.classes);
  }
  launch_export_pack(s, e);
  LMX_HIP(hipGetLastError());
  // the slot is not reused before this, and the caller's stream goes on behind it
  LMX_HIP(hipEventRecord(c->export_done[slot], s));
  c->export_pending[slot] = true;
  LMX_HIP(hipStreamWaitEvent(user, c->export_done[slot], 0));
  return LMX_OK;
}

lmx_status lmx_ctx_export_matches_on(lmx_ctx* c, int32_t n_frames, const lmx_export_desc* d, void* stream) {
  return lmx::guarded("lmx_ctx_export_matches_on", [&]() -> lmx_status {
  const char* const what = "lmx_ctx_export_matches_on";
  if (!c || !d) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  if (d->struct_size != sizeof(lmx_export_desc)) { set_error("%s: struct_size %u, not %zu", what, d->struct_size, sizeof(lmx_export_desc)); return LMX_ERR_INVALID_ARG; }
  ExportRequest q{};
  q.oldest = d->oldest; q.max_large_frames = d->max_large_frames; q.clusters = d->clusters != 0;
  q.header = d->header; q.frame_info = d->frame_info; q.matches = d->matches; q.cap_matches = d->cap_matches;
  q.clusters_out = d->clusters_out; q.cap_clusters = d->cap_clusters; q.members = d->members; q.cap_members = d->cap_members;
  return export_impl(what, c, n_frames, q, stream);
  });
}

lmx_status lmx_ctx_export_clusters_on(lmx_ctx* c, int32_t n_frames, const lmx_export_clusters_desc* d, void* stream) {
  return lmx::guarded("lmx_ctx_export_clusters_on", [&]() -> lmx_status {
  const char* const what = "lmx_ctx_export_clusters_on";
  if (!c || !d) { set_error("%s: null argument", what); return LMX_ERR_INVALID_ARG; }
  if (d->struct_size != sizeof(lmx_export_clusters_desc)) { set_error("%s: struct_size %u, not %zu", what, d->struct_size, sizeof(lmx_export_clusters_desc)); return LMX_ERR_INVALID_ARG; }
  if (d->score < 0 || d->score > 2) { set_error("%s: score %d outside 0 .. 2", what, d->score); return LMX_ERR_INVALID_ARG; }
  if (d->classes < 0 || d->classes > 1) { set_error("%s: classes %d outside 0 .. 1", what, d->classes); return LMX_ERR_INVALID_ARG; }
  ExportRequest q{};
  q.oldest = d->oldest; q.max_large_frames = d->max_large_frames; q.clusters = true; q.classes = d->classes == 1; q.score = (F2Score)d->score;   // the same 0 / 1 / 2, checked above
  q.templates = d->templates; q.class_index = d->classes ? -1 : d->class_index; q.class_base = d->class_base; q.n_classes = d->n_classes; q.no_value = d->no_value;
  q.header = d->header; q.frame_info = d->frame_info; q.matches = d->matches; q.cap_matches = d->cap_matches;
  q.diffs = d->diffs; q.ndiffs = d->ndiffs; q.clusters_out = d->clusters_out; q.cap_clusters = d->cap_clusters; q.cluster_class = d->cluster_class;
  q.members = d->members; q.cap_members = d->cap_members;
  return export_impl(what, c, n_frames, q, stream);
  });
}

lmx_status lmx_ctx_export_raw(lmx_ctx* c, void* d_block, size_t capacity_records) {
  return lmx_ctx_export_raw_on(c, d_block, capacity_records, c ? (void*)c->stream : nullptr);
}

int32_t lmx_ctx_max_outstanding(const lmx_ctx* c) { return c ? c->n_slots : 0; }

lmx_status lmx_ctx_release(lmx_ctx* c) {
  if (!c) { set_error("lmx_ctx_release: null context"); return LMX_ERR_INVALID_ARG; }
  if (c->outstanding < 1) { set_error("lmx_ctx_release: nothing enqueued"); return LMX_ERR_INVALID_ARG; }
  LMX_HIP(hipSetDevice(c->device));
  const int slot = (c->head + c->n_slots - c->outstanding) % c->n_slots;
  LMX_HIP(hipEventSynchronize(c->done[slot]));
  if (lmx_status xs = wait_exports(c, slot)) return xs;   // a released slot is never read by a still-running export
  c->outstanding -= 1;
  if (c->outstanding == 0) drain_profiling(c);
  // the counters lmx_ctx_stats reports, as collect leaves them: the slot's pinned mirror holds the published header once its event has
  // completed (the sharded callers consume the records on the device and never collect; round 3 reported 0 candidates for them)
  const uint32_t* h_hdr = reinterpret_cast<const uint32_t*>(c->h_out_slot[slot]);
  c->stat_cands = h_hdr[0]; c->stat_matches = h_hdr[1];
  return LMX_OK;
}

lmx_status lmx_stream_copy(void* dst, const void* src, size_t bytes, void* stream) {
  if (!dst || !src) { set_error("lmx_stream_copy: null argument"); return LMX_ERR_INVALID_ARG; }
  if (((uintptr_t)dst | (uintptr_t)src | bytes) & 15u) { set_error("lmx_stream_copy: pointers and size must be multiples of 16 bytes"); return LMX_ERR_INVALID_ARG; }
  launch_copy_bytes((hipStream_t)stream, dst, src, bytes);
  LMX_HIP(hipGetLastError());
  return LMX_OK;
}

lmx_status lmx_stream_copy_blocks(void* dst, const void* src, int32_t n_blocks, size_t block_stride_bytes, size_t capacity_records, void* stream) {
  if (!dst || !src || n_blocks < 1) { set_error("lmx_stream_copy_blocks: invalid argument"); return LMX_ERR_INVALID_ARG; }
  if ((((uintptr_t)dst | (uintptr_t)src | block_stride_bytes) & 15u) || block_stride_bytes < LMX_GATHER_HEADER_BYTES + capacity_records * sizeof(lmx_raw_match_t)) {
    set_error("lmx_stream_copy_blocks: pointers and stride must be multiples of 16 bytes and a block must hold its capacity");
    return LMX_ERR_INVALID_ARG;
  }
  launch_publish_blocks((hipStream_t)stream, dst, src, n_blocks, block_stride_bytes, (uint32_t)std::min<size_t>(capacity_records, 0xffffffffu));
  LMX_HIP(hipGetLastError());
  return LMX_OK;
}

lmx_status lmx_merge_gathered_groups(const void* blocks, int32_t n_ranks, size_t block_stride_bytes, size_t capacity_records, int32_t n_frames,
                                     int32_t frame_groups, lmx_match_t* out, size_t cap_total, size_t* offsets) {
  return lmx::guarded("lmx_merge_gathered", [&]() -> lmx_status {
  if (!blocks || !offsets || n_ranks < 1 || n_frames < 1 || (cap_total > 0 && !out)) { set_error("lmx_merge_gathered: invalid argument"); return LMX_ERR_INVALID_ARG; }
  const int G = frame_groups < 1 ? 1 : frame_groups;
  if (n_ranks % G != 0) { set_error("lmx_merge_gathered_groups: %d ranks do not form %d frame groups", n_ranks, G); return LMX_ERR_INVALID_ARG; }
  const int R = n_ranks / G;
  std::vector<std::vector<const lmx_raw_match_t*>> per_frame(n_frames);
  for (int r = 0; r < n_ranks; ++r) {
    const uint8_t* blk = (const uint8_t*)blocks + (size_t)r * block_stride_bytes;
    const uint32_t n = reinterpret_cast<const uint32_t*>(blk)[1];
    const uint32_t n_cand = reinterpret_cast<const uint32_t*>(blk)[0], cand_cap = reinterpret_cast<const uint32_t*>(blk)[2];
    if (cand_cap != 0 && n_cand > cand_cap) {
      // the rank's scoring kernel dropped candidates (which ones is not deterministic): its matches are incomplete
      for (int f = 0; f <= n_frames; ++f) offsets[f] = 0;
      set_error("rank %d: candidate list overflow (%u candidates > capacity %u); raise lmx_ctx_desc.max_candidates", r, n_cand, cand_cap);
      return LMX_ERR_OVERFLOW;
    }
    if (n > capacity_records) {
      for (int f = 0; f <= n_frames; ++f) offsets[f] = 0;
      set_error("rank %d wrote %u records > gather capacity %zu", r, n, capacity_records);
      return LMX_ERR_OVERFLOW;
    }
    // the rank's frames within the batch: its frame group's slice (the whole batch when G == 1); record frames are local to it
    const int g = r / R;
    const int f_begin = (int)((long)g * n_frames / G), f_count = (int)((long)(g + 1) * n_frames / G) - f_begin;
    const lmx_raw_match_t* recs = reinterpret_cast<const lmx_raw_match_t*>(blk + LMX_GATHER_HEADER_BYTES);
    for (uint32_t i = 0; i < n; ++i)
      if (recs[i].frame >= 0 && recs[i].frame < f_count) per_frame[f_begin + recs[i].frame].push_back(&recs[i]);
  }
  size_t pos = 0;
  offsets[0] = 0;
  std::vector<HostMatch> fin;
  for (int f = 0; f < n_frames; ++f) {
    finalize_frame(per_frame[f], fin);
    for (size_t i = 0; i < fin.size(); ++i, ++pos)
      if (pos < cap_total) out[pos] = fin[i].m;
    offsets[f + 1] = pos;
  }
  if (pos > cap_total) { set_error("%zu matches > output capacity %zu", pos, cap_total); return LMX_ERR_OVERFLOW; }
  return LMX_OK;
  });
}

lmx_status lmx_merge_gathered(const void* blocks, int32_t n_ranks, size_t block_stride_bytes, size_t capacity_records, int32_t n_frames,
                              lmx_match_t* out, size_t cap_total, size_t* offsets) {
  return lmx_merge_gathered_groups(blocks, n_ranks, block_stride_bytes, capacity_records, n_frames, 1, out, cap_total, offsets);
}

lmx_status lmx_ctx_sync(lmx_ctx* c) {
  if (!c) { set_error("lmx_ctx_sync: null context"); return LMX_ERR_INVALID_ARG; }
  LMX_HIP(hipSetDevice(c->device));
  if (sync_lanes(c) != LMX_OK) return LMX_ERR_HIP;
  drain_profiling(c);
  c->outstanding = 0;  // abandons enqueues that were not collected (their results stay readable via export_raw)
  return LMX_OK;
}

lmx_status lmx_merge_raw(const lmx_raw_match_t* records, size_t n_records, lmx_match_t* out, size_t cap, size_t* n_out) {
  return lmx::guarded("lmx_merge_raw", [&]() -> lmx_status {
  if ((n_records > 0 && !records) || !n_out || (cap > 0 && !out)) { set_error("lmx_merge_raw: null argument"); return LMX_ERR_INVALID_ARG; }
  std::vector<const lmx_raw_match_t*> recs(n_records);
  for (size_t i = 0; i < n_records; ++i) recs[i] = &records[i];
  std::vector<HostMatch> fin;
  finalize_frame(recs, fin);
  *n_out = fin.size();
  const size_t n = std::min(cap, fin.size());
  for (size_t i = 0; i < n; ++i) out[i] = fin[i].m;
  if (fin.size() > cap) { set_error("%zu matches > output capacity %zu", fin.size(), cap); return LMX_ERR_OVERFLOW; }
  return LMX_OK;
  });
}

}  // extern "C"
