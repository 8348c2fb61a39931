// include/lmx_linemod.hpp -- header-only C++ facade over the C ABI (include/lmx.h) that keeps the names and
// semantics of cv::linemod as the reference uses them, so a maintainer can swap the body of
//   rgbdDetector::linemod_detection   (/root/reference/src/rgbdDetector.cpp:31-34)
// and of readLinemod                  (/root/reference/src/rgbdDetector.cpp:1668-1680)
// without touching src/linemod_ensenso_detect_*.cpp.  See INTEGRATION.md for the exact edit.
//
//   lmx::linemod::Feature / Template / Match      <-> cv::linemod::Feature / Template / Match
//   lmx::linemod::Detector::match(sources, threshold, matches, class_ids)
//                                                <-> cv::linemod::Detector::match(sources, threshold, matches, class_ids, noArray())
//   Detector::read / classIds / getTemplates / numTemplates / getT / pyramidLevels: same meaning as upstream.
// Errors: any non-OK lmx_status throws lmx::linemod::Exception (the analogue of the cv::Exception a CV_Assert throws).
// With LMX_HAVE_OPENCV defined, overloads taking cv::Mat are provided (the only place OpenCV types appear).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "lmx.h"

#ifdef LMX_HAVE_OPENCV
#include <opencv2/core/core.hpp>
#endif

namespace lmx {
namespace linemod {

struct Exception : std::runtime_error {
  lmx_status status;
  Exception(lmx_status s, const char* what) : std::runtime_error(what), status(s) {}
};

inline void check(lmx_status s) {
  if (s != LMX_OK) throw Exception(s, lmx_last_error());
}

struct Feature {
  int x, y, label;
};

struct Template {
  int width, height, pyramid_level;
  std::vector<Feature> features;
};

struct Match {
  Match() : x(0), y(0), similarity(0), template_id(0) {}
  Match(int x_, int y_, float s, const std::string& c, int t) : x(x_), y(y_), similarity(s), class_id(c), template_id(t) {}
  bool operator<(const Match& rhs) const {
    if (similarity != rhs.similarity) return similarity > rhs.similarity;
    return template_id < rhs.template_id;
  }
  bool operator==(const Match& rhs) const {
    return x == rhs.x && y == rhs.y && similarity == rhs.similarity && class_id == rhs.class_id;
  }
  int x, y;
  float similarity;
  std::string class_id;
  int template_id;
};

// Non-owning image view (what cv::Mat carries for this path).
struct Image {
  const void* data;
  int rows, cols, channels, elem_size;
  size_t step;
  lmx_image c() const { return lmx_image{data, rows, cols, channels, elem_size, step}; }
};

class DepthTemplates;

// What Detector::collectClustersClasses returns: frame f's matches are matches[match_offsets[f] .. match_offsets[f + 1]) (diffs / ndiffs
// parallel to them, empty without a score / without normals), its clusters clusters[cluster_offsets[f] .. cluster_offsets[f + 1]) with
// cluster_class[k] the class of clusters[k]; a cluster's members are members[member_begin .. member_begin + member_count), indices into
// its frame's matches.
struct ClassClusters {
  std::vector<lmx_match_t> matches;
  std::vector<lmx_depth_diff_t> diffs;
  std::vector<lmx_normal_diff_t> ndiffs;
  std::vector<lmx_cluster_t> clusters;
  std::vector<int32_t> cluster_class, members;
  std::vector<size_t> match_offsets, cluster_offsets;
};

class Detector {
 public:
  Detector() {}
  ~Detector() { reset(); }
  Detector(const Detector&) = delete;
  Detector& operator=(const Detector&) = delete;

  // readLinemod(filename): FileStorage YAML -> Detector::read + readClass per class
  void read(const std::string& filename) {
    reset();
    // through the library's file cache (parsed once per (path, mtime, size), binary side file for the next process); this detector gets a
    // private copy it may modify: ~1 ms for 3000 templates instead of the 0.13-0.24 s parse on every read of the same file
    const lmx_bank* cached = nullptr;
    check(lmx_bank_load_yaml_cached(filename.c_str(), &cached));
    const lmx_status st = lmx_bank_clone(cached, &bank_);
    lmx_bank_release(cached);
    check(st);
  }
  void write(const std::string& filename) const { check(lmx_bank_save_yaml(bank_, filename.c_str())); }

  // A detector that starts empty: cv::linemod::Detector(modalities, T) as the reference's trainers build it (src/renderer.cpp:179-185).
  void create(const std::vector<lmx_modality_desc>& modalities, const std::vector<int>& T) {
    reset();
    std::vector<int32_t> t(T.begin(), T.end());
    lmx_bank_desc d;
    d.pyramid_levels = (int32_t)t.size(); d.T = t.data(); d.n_modalities = (int32_t)modalities.size(); d.modalities = modalities.data();
    check(lmx_bank_create(&d, &bank_));
  }

  // The trainer loop of src/renderer.cpp:262-329 (lmx_bank_train_mesh): renders `triangles` ([n][3][3] doubles, metres) from every view on
  // the device and adds a template per view addTemplate accepts, in view order.  -> the template id per view (-1: rejected).  `side_car`
  // (may be null) receives the renderer-params side-car of the accepted views; free it with lmx_renderer_params_free.
  std::vector<int> addTemplatesFromMesh(const std::vector<double>& triangles, const lmx_mesh_camera& camera, const std::vector<lmx_mesh_view>& views,
                                        const std::string& class_id, lmx_renderer_params** side_car = nullptr,
                                        const lmx_train_mesh_opts* opts = nullptr /* e.g. candidates = LMX_TRAIN_CANDIDATES_DEVICE; null: the host path */,
                                        lmx_train_mesh_stats* stats = nullptr) {
    if (triangles.size() % 9 != 0) throw Exception(LMX_ERR_SHAPE, "addTemplatesFromMesh: triangles must hold 9 doubles per triangle");
    std::vector<int32_t> ids(views.size(), -1);
    check(lmx_bank_train_mesh_opts(bank_, device_, triangles.data(), (int32_t)(triangles.size() / 9), &camera, views.data(), (int32_t)views.size(),
                                   class_id.c_str(), ids.data(), side_car, opts, stats));
    return std::vector<int>(ids.begin(), ids.end());
  }

  // Device placement (no upstream analogue).  Called lazily by match() with the frame size of the first call.
  void setDevice(int device, int max_batch = 1, int max_candidates = 0, void* stream = nullptr) {
    device_ = device; max_batch_ = max_batch; max_candidates_ = max_candidates; stream_ = stream;
  }

  std::vector<std::string> classIds() const {
    std::vector<std::string> ids;
    for (int i = 0; i < lmx_bank_num_classes(bank_); ++i) ids.push_back(lmx_bank_class_id(bank_, i));
    return ids;
  }
  int numTemplates() const { return lmx_bank_num_templates(bank_, nullptr); }
  int numTemplates(const std::string& class_id) const { return lmx_bank_num_templates(bank_, class_id.c_str()); }
  int numClasses() const { return lmx_bank_num_classes(bank_); }
  int getT(int pyramid_level) const { return lmx_bank_T(bank_, pyramid_level); }
  int pyramidLevels() const { return lmx_bank_pyramid_levels(bank_); }

  std::vector<Template> getTemplates(const std::string& class_id, int template_id) const {
    const int per = lmx_bank_pyramid_levels(bank_) * lmx_bank_num_modalities(bank_);
    std::vector<Template> out(per);
    for (int k = 0; k < per; ++k) {
      const int32_t* f = nullptr;
      int32_t n = 0, w = 0, h = 0, l = 0;
      check(lmx_bank_get_template(bank_, class_id.c_str(), template_id, k, &w, &h, &l, &f, &n));
      out[k].width = w; out[k].height = h; out[k].pyramid_level = l;
      for (int i = 0; i < n; ++i) out[k].features.push_back(Feature{f[3 * i], f[3 * i + 1], f[3 * i + 2]});
    }
    return out;
  }

  // Detector::match.  `matches` is cleared first, like upstream.
  void match(const std::vector<Image>& sources, float threshold, std::vector<Match>& matches,
             const std::vector<std::string>& class_ids = std::vector<std::string>()) {
    match_any(sources, threshold, nullptr, matches, class_ids);
  }
  // liblmx extension (no upstream analogue): a threshold per class (lmx_match_thresholds).  The map's keys are the classes matched, in map
  // order -- upstream's order for an empty class_ids -- each at its own threshold, as if Detector::match passed thresholds[class] to every
  // matchClass call; one std::sort + std::unique over everything.  A key the bank does not hold throws; an empty map matches nothing.
  void match(const std::vector<Image>& sources, const std::map<std::string, float>& thresholds, std::vector<Match>& matches) {
    matches.clear();
    if (thresholds.empty()) return;
    std::vector<std::string> ids;
    const std::vector<float> thr = class_thresholds(thresholds, &ids);
    match_any(sources, 0.f, &thr, matches, ids);
  }

 private:
  // the map as lmx_ctx_enqueue_thresholds takes it: one entry per class index (classes the map lacks are not matched, their entry is not
  // read), and the keys in map order as the class_ids list
  std::vector<float> class_thresholds(const std::map<std::string, float>& thresholds, std::vector<std::string>* ids) const {
    const std::vector<std::string> known = classIds();
    std::vector<float> thr(known.size(), 0.f);
    for (const std::pair<const std::string, float>& kv : thresholds) {
      size_t k = 0;
      while (k < known.size() && known[k] != kv.first) ++k;
      if (k == known.size()) throw Exception(LMX_ERR_INVALID_ARG, ("match: a threshold for class \"" + kv.first + "\", which the detector does not hold").c_str());
      thr[k] = kv.second;
      ids->push_back(kv.first);
    }
    return thr;
  }
  void match_any(const std::vector<Image>& sources, float threshold, const std::vector<float>* thresholds, std::vector<Match>& matches,
                 const std::vector<std::string>& class_ids) {
    matches.clear();
    if (sources.empty()) throw Exception(LMX_ERR_SHAPE, "match: no sources");
    std::vector<lmx_image> imgs;
    for (const Image& s : sources) imgs.push_back(s.c());
    std::vector<const char*> cids;
    for (const std::string& c : class_ids) cids.push_back(c.c_str());
    if (buf_.size() < 4096) buf_.resize(4096);
    // a one-channel 8-bit source can only be a gray ColorGradient frame (depth is 16-bit): it is matched on a gray context (LMX_CTX_GRAY),
    // with the matches of the frame copied into B, G and R.  Gray and BGR calls may alternate: each kind keeps a context of its own.
    bool gray = false;
    for (const Image& s : sources) gray = gray || (s.channels == 1 && s.elem_size == 1);
    for (int attempt = 0;; ++attempt) {
      ensure_ctx(sources[0].cols, sources[0].rows, gray);
      size_t n = 0;
      lmx_status st = thresholds ? lmx_match_thresholds(ctx_, imgs.data(), (int)imgs.size(), thresholds->data(), (int32_t)thresholds->size(), cids.data(), (int)cids.size(),
                                                        buf_.data(), buf_.size(), &n)
                                 : lmx_match(ctx_, imgs.data(), (int)imgs.size(), threshold, cids.empty() ? nullptr : cids.data(), (int)cids.size(),
                                             buf_.data(), buf_.size(), &n);
      if (st == LMX_ERR_OVERFLOW && n > buf_.size()) { buf_.resize(n); continue; }  // output buffer too small: retry
      if (st == LMX_ERR_OVERFLOW && attempt < 8) {
        // the device's candidate / match lists overflowed (upstream has no such limit): rebuild the context with lists sized from
        // the counts the failed call reports, and repeat the call
        int64_t n_cand = 0, n_raw = 0;
        check(lmx_ctx_stats(ctx_, &n_cand, &n_raw));
        const int64_t need = (n_cand > n_raw ? n_cand : n_raw) / (max_batch_ > 0 ? max_batch_ : 1) + 1024;
        int grown = max_candidates_ > 16384 ? max_candidates_ : 16384;
        while (grown < need && grown < (1 << 26)) grown *= 2;
        if (grown > max_candidates_ && grown > 16384) {
          max_candidates_ = grown;
          lmx_ctx_destroy(ctx_); ctx_ = nullptr; slot_[gray] = nullptr;
          continue;
        }
      }
      check(st);
      for (size_t i = 0; i < n; ++i)
        matches.push_back(Match(buf_[i].x, buf_[i].y, buf_[i].similarity, lmx_bank_class_id(bank_, buf_[i].class_index), buf_[i].template_id));
      return;
    }
  }

 public:
#ifdef LMX_HAVE_OPENCV
  static Image view(const cv::Mat& m) { return Image{m.data, m.rows, m.cols, m.channels(), (int)m.elemSize1(), m.step[0]}; }
  void match(const std::vector<cv::Mat>& sources, float threshold, std::vector<Match>& matches,
             const std::vector<std::string>& class_ids = std::vector<std::string>()) {
    std::vector<Image> v;
    for (const cv::Mat& m : sources) v.push_back(view(m));
    match(v, threshold, matches, class_ids);
  }
  void match(const std::vector<cv::Mat>& sources, const std::map<std::string, float>& thresholds, std::vector<Match>& matches) {
    std::vector<Image> v;
    for (const cv::Mat& m : sources) v.push_back(view(m));
    match(v, thresholds, matches);
  }
#endif

  // The two-detector node as one bank of two classes.  Class class_index's `<object>_renderer_params.yml`
  // side-car and clustering parameters for the per-class consumer chain (lmx_ctx_set_cluster_sidecar_class); class_index is the position
  // of the class in classIds(), 0 .. 15; empty vectors remove it.  Kept with the detector and handed to its context whenever one is made.
  void setClusterSidecar(int class_index, const std::vector<double>& obj_origin_dists, const std::vector<int32_t>& rects, const lmx_cluster_params& params) {
    if (rects.size() != obj_origin_dists.size() * 4) throw Exception(LMX_ERR_SHAPE, "setClusterSidecar: four rect values per origin distance");
    if (class_index < 0 || class_index >= 16) throw Exception(LMX_ERR_INVALID_ARG, "setClusterSidecar: class_index must be 0 .. 15 (lmx_cluster_matches_classes on the host takes any number)");
    if (slot_[0]) check(lmx_ctx_set_cluster_sidecar_class(slot_[0], class_index, obj_origin_dists.data(), rects.data(), obj_origin_dists.size(), &params));
    sidecars_[class_index] = ClassSidecar{obj_origin_dists, rects, params};
  }
  // One batch of BGR (+ depth) frames through match and the per-class chain in one enqueue and one collect
  // (lmx_ctx_collect_clusters_classes): frames[f] holds frame f's sources; setDevice's max_batch must cover frames.size().  templates
  // null: clusters ranked by mean similarity.  Else the object holds every class's crops, class c's at class_base[c] .. class_base[c + 1]
  // (DepthTemplates::append), depth[f] is frame f's 16-bit depth image and the score is the depth difference, with normals the normal term
  // too.  Per class the result is lmx_cluster_matches on that class's matches of the joined list; it is not bit for bit what two
  // single-class detectors give (include/lmx.h, "What this is NOT").  The call collects the context's OLDEST outstanding enqueue and, when
  // the collect is refused, releases the oldest one: use it on a context that has nothing outstanding (one driven through context() and
  // the C API with an enqueue of its own in flight would get, or lose, that one).  Defined behind DepthTemplates.
  ClassClusters collectClustersClasses(const std::vector<std::vector<Image> >& frames, float threshold, DepthTemplates* templates = nullptr,
                                       const std::vector<int32_t>& class_base = std::vector<int32_t>(), const std::vector<Image>& depth = std::vector<Image>(),
                                       bool normals = false, double no_value = -HUGE_VAL, size_t capacity = 1 << 16);
  // The same with a threshold per class in front of the chain (see the match overload): the map's keys are the classes matched
  ClassClusters collectClustersClasses(const std::vector<std::vector<Image> >& frames, const std::map<std::string, float>& thresholds,
                                       DepthTemplates* templates = nullptr, const std::vector<int32_t>& class_base = std::vector<int32_t>(),
                                       const std::vector<Image>& depth = std::vector<Image>(), bool normals = false, double no_value = -HUGE_VAL,
                                       size_t capacity = 1 << 16);

  // Frames that already live in device memory, on the context's device (lmx_ctx_upload_device; include/lmx.h has the ordering contract):
  // every Image's data is a device pointer, `stream` the stream that produced the frames (null: the null stream).  Without `pre` the
  // sources are frame-sized (a context of their size is created if there is none); with it they go through the node-side steps of
  // lmx_ctx_upload_raw into the current context.  Enqueue and collect through context() as after any upload.
  void uploadDevice(const std::vector<std::vector<Image> >& frames, const lmx_pre_desc* pre = nullptr, void* stream = nullptr) {
    if (frames.empty() || frames[0].empty()) throw Exception(LMX_ERR_SHAPE, "uploadDevice: no frames");
    std::vector<lmx_image> imgs;
    for (const std::vector<Image>& f : frames) {
      if (f.size() != frames[0].size()) throw Exception(LMX_ERR_SHAPE, "uploadDevice: every frame needs the same sources");
      for (const Image& s : f) imgs.push_back(s.c());
    }
    if (!pre) ensure_ctx(frames[0][0].cols, frames[0][0].rows, false);
    else if (!ctx_) throw Exception(LMX_ERR_INVALID_ARG, "uploadDevice: raw frames need a context of the cropped size first");
    check(lmx_ctx_upload_device(ctx_, (int32_t)frames.size(), imgs.data(), (int32_t)frames[0].size(), pre, stream));
    uploaded_frames_ = (int32_t)frames.size();
  }

  // The way out for a next stage on the GPU (lmx_ctx_export_matches_on; include/lmx.h has the layout and the ordering contract): the final
  // matches -- with desc.clusters the clusters and members too -- of the current context's most recent (desc.oldest: oldest outstanding)
  // enqueue into the caller's device arrays, valid for work queued on `stream` (null: the null stream) after the call.  Nothing waits on the
  // host and the enqueue stays outstanding: lmx_ctx_release(context()) or a collect ends it.  desc.struct_size is the caller's to set.
  // n_frames is the enqueue's frame count; 0: as many as the last uploadDevice brought.
  void exportMatches(const lmx_export_desc& desc, void* stream = nullptr, int32_t n_frames = 0) {
    if (!ctx_) throw Exception(LMX_ERR_INVALID_ARG, "exportMatches: no context, nothing was enqueued");
    check(lmx_ctx_export_matches_on(ctx_, n_frames > 0 ? n_frames : uploaded_frames_, &desc, stream));
  }

  // exportMatches for every cluster chain (lmx_ctx_export_clusters_on): desc.classes picks the un-classed or the per-class side-cars,
  // desc.score mean similarity, the depth score or depth + normal against desc.templates (DepthTemplates::handle(), whose
  // uploadScene / uploadSceneDevice followed the enqueue); diffs, ndiffs and cluster_class arrive next to the matches and clusters.
  // Stream, frame count and the enqueue's fate as for exportMatches; desc.struct_size is the caller's to set.
  void exportClusters(const lmx_export_clusters_desc& desc, void* stream = nullptr, int32_t n_frames = 0) {
    if (!ctx_) throw Exception(LMX_ERR_INVALID_ARG, "exportClusters: no context, nothing was enqueued");
    check(lmx_ctx_export_clusters_on(ctx_, n_frames > 0 ? n_frames : uploaded_frames_, &desc, stream));
  }

  lmx_bank* bank() const { return bank_; }
  lmx_ctx* context() const { return ctx_; }
  // Which path completed the frames of the context's last lmx_ctx_collect_clusters* call, collectClustersClasses included
  // (lmx_ctx_chain_stats: LDS kernel, large-frame kernel, host); zeros before a context exists
  lmx_chain_stats chainStats() const {
    lmx_chain_stats s = lmx_chain_stats();
    if (ctx_) check(lmx_ctx_chain_stats(ctx_, &s));
    return s;
  }

 private:
  ClassClusters collect_clusters_classes(const std::vector<std::vector<Image> >& frames, float threshold, const std::map<std::string, float>* thresholds,
                                         DepthTemplates* templates, const std::vector<int32_t>& class_base, const std::vector<Image>& depth, bool normals,
                                         double no_value, size_t capacity);
  struct ClassSidecar { std::vector<double> dists; std::vector<int32_t> rects; lmx_cluster_params params; };
  std::map<int, ClassSidecar> sidecars_;
  void reset() {
    for (int k = 0; k < 2; ++k)
      if (slot_[k]) lmx_ctx_destroy(slot_[k]);
    if (bank_) lmx_bank_destroy(bank_);
    slot_[0] = slot_[1] = nullptr; ctx_ = nullptr; bank_ = nullptr;
  }
  // ctx_ = the context of the current call: slot_[0] for BGR sources, slot_[1] for gray ones (LMX_CTX_GRAY)
  void ensure_ctx(int w, int h, bool gray) {
    lmx_ctx*& c = slot_[gray ? 1 : 0];
    if (c && (w != w_[gray] || h != h_[gray])) { lmx_ctx_destroy(c); c = nullptr; }
    if (!c) {
      lmx_ctx_desc d;
      std::memset(&d, 0, sizeof(d));
      d.device = device_; d.width = w; d.height = h; d.max_batch = max_batch_; d.max_candidates = max_candidates_; d.stream = stream_;
      d.flags = gray ? LMX_CTX_GRAY : 0;
      check(lmx_ctx_create(bank_, &d, &c));
      w_[gray] = w; h_[gray] = h;
      if (!gray)
        for (const std::pair<const int, ClassSidecar>& k : sidecars_)
          check(lmx_ctx_set_cluster_sidecar_class(c, k.first, k.second.dists.data(), k.second.rects.data(), k.second.dists.size(), &k.second.params));
    }
    ctx_ = c;
  }
  lmx_bank* bank_ = nullptr;
  lmx_ctx* ctx_ = nullptr;
  lmx_ctx* slot_[2] = {nullptr, nullptr};
  int device_ = 0, max_batch_ = 1, max_candidates_ = 0, w_[2] = {0, 0}, h_[2] = {0, 0};
  void* stream_ = nullptr;
  int32_t uploaded_frames_ = 0;   // of the last uploadDevice: exportMatches' default frame count
  std::vector<lmx_match_t> buf_;
};

// Device-resident depth renders of a bank's templates and the depth check of matches against them (lmx_depth_templates_*,
// lmx_depth_diff_matches): the depth half of rgbdDetector::depth_normal_diff_calc (src/rgbdDetector.cpp:147-282) without its per-match
// re-render.  Template ids are the bank's: with fromMesh, views[i] is template i's view (side_car->R[i], side_car->T[i][2] of
// Detector::addTemplatesFromMesh).
class DepthTemplates {
 public:
  DepthTemplates() {}
  ~DepthTemplates() { reset(); }
  DepthTemplates(const DepthTemplates&) = delete;
  DepthTemplates& operator=(const DepthTemplates&) = delete;
  DepthTemplates(DepthTemplates&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  DepthTemplates& operator=(DepthTemplates&& o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }

  void fromMesh(const std::vector<double>& triangles, const lmx_mesh_camera& camera, const std::vector<lmx_mesh_view>& views, int device = 0) {
    if (triangles.size() % 9 != 0) throw Exception(LMX_ERR_SHAPE, "DepthTemplates::fromMesh: triangles must hold 9 doubles per triangle");
    reset();
    check(lmx_depth_templates_from_mesh(device, triangles.data(), (int32_t)(triangles.size() / 9), &camera, views.data(), (int32_t)views.size(), &h_));
  }
  // crops[i]: sizes[i].first x sizes[i].second (width x height) uint16 millimetres, dense rows, 0 = not on the object
  void fromCrops(const std::vector<const uint16_t*>& crops, const std::vector<std::pair<int, int> >& sizes, int device = 0) {
    if (crops.size() != sizes.size()) throw Exception(LMX_ERR_SHAPE, "DepthTemplates::fromCrops: one size per crop");
    std::vector<int32_t> wh;
    for (const std::pair<int, int>& s : sizes) { wh.push_back(s.first); wh.push_back(s.second); }
    reset();
    check(lmx_depth_templates_from_crops(device, crops.data(), wh.data(), (int32_t)crops.size(), &h_));
  }
  int count() const { return lmx_depth_templates_count(h_); }
  size_t deviceBytes() const { return lmx_depth_templates_device_bytes(h_); }

  // One frame: out[i] belongs to matches[i] ({sum_abs_mm, n_valid, n_template}; mean difference in mm = sum_abs_mm / n_valid).
  // class_index >= 0: only that class's matches are looked at, the others get zeros.
  std::vector<lmx_depth_diff_t> diff(const Image& depth, const std::vector<lmx_match_t>& matches, int class_index = -1) {
    std::vector<lmx_depth_diff_t> out(matches.size());
    const lmx_image img = depth.c();
    const size_t offsets[2] = {0, matches.size()};
    check(lmx_depth_diff_matches(h_, &img, 1, matches.data(), offsets, class_index, out.data()));
    return out;
  }
  // A batch: frame f's matches are matches[offsets[f] .. offsets[f + 1]).
  std::vector<lmx_depth_diff_t> diff(const std::vector<Image>& depth, const std::vector<lmx_match_t>& matches, const std::vector<size_t>& offsets,
                                     int class_index = -1) {
    if (offsets.size() != depth.size() + 1 || offsets.back() != matches.size()) throw Exception(LMX_ERR_SHAPE, "DepthTemplates::diff: offsets must hold one entry per frame plus one and end at matches.size()");
    std::vector<lmx_image> imgs;
    for (const Image& d : depth) imgs.push_back(d.c());
    std::vector<lmx_depth_diff_t> out(matches.size());
    check(lmx_depth_diff_matches(h_, imgs.data(), (int32_t)imgs.size(), matches.data(), offsets.data(), class_index, out.data()));
    return out;
  }
  // The value lmx_cluster_matches_scored and collectClustersDepth rank by: minus the mean difference in metres (no_value when nothing
  // could be compared).
  static double value(const lmx_depth_diff_t& d, double no_value = -HUGE_VAL) { return lmx_depth_value(&d, no_value); }

  // Pose refinement (lmx_pose_refine_matches, the reference's icpPoseRefine stage): out[i] belongs to matches[i]; R, t_mm map a point of
  // the matched template's view (model camera frame, mm) into the scene camera frame.  params.struct_size is filled in here.  With
  // `depth` one frame holding all matches; without, the scene uploadScene left in the object (one frame).
  std::vector<lmx_pose_refine_t> refinePoses(const std::vector<lmx_match_t>& matches, lmx_pose_refine_params params, const Image* depth = nullptr,
                                             int class_index = -1) {
    std::vector<lmx_pose_refine_t> out(matches.size());
    params.struct_size = (uint32_t)sizeof(lmx_pose_refine_params);
    const size_t offsets[2] = {0, matches.size()};
    lmx_image img;
    if (depth) img = depth->c();
    check(lmx_pose_refine_matches(h_, depth ? &img : nullptr, 1, matches.data(), offsets, class_index, &params, out.data()));
    return out;
  }
  std::vector<lmx_pose_refine_t> refinePoses(const std::vector<lmx_match_t>& matches, const lmx_pose_refine_params& params, const Image& depth,
                                             int class_index = -1) {
    return refinePoses(matches, params, &depth, class_index);
  }
  // The parameters with the defaults of the Python front end; the cameras are the caller's to fill.
  static lmx_pose_refine_params poseRefineDefaults() {
    lmx_pose_refine_params p = lmx_pose_refine_params();
    p.struct_size = (uint32_t)sizeof(lmx_pose_refine_params);
    p.max_dist_mm = 10.0; p.eps_rot_rad = 1e-5; p.eps_trans_mm = 1e-3;
    p.max_iterations = 20; p.min_pairs = 16; p.search_radius = 1;
    return p;
  }
  // The refinement schedule of this object (lmx_depth_templates_set_refine_schedule): 1 to 4 stages, each with its own correspondence
  // distance, stopping rule, window and stride, fed into one another; an empty vector clears it.  While one is set, refinePoses and the
  // chains refine by it and take the cameras, min_pairs and rects from their own parameters.
  void setRefineSchedule(const std::vector<lmx_pose_refine_stage>& stages) {
    check(lmx_depth_templates_set_refine_schedule(h_, stages.empty() ? nullptr : stages.data(), (int32_t)stages.size()));
  }
  std::vector<lmx_pose_refine_stage> refineSchedule() const {
    lmx_pose_refine_stage out[LMX_POSE_MAX_STAGES];
    int32_t n = 0;
    check(lmx_depth_templates_get_refine_schedule(h_, out, &n));
    return std::vector<lmx_pose_refine_stage>(out, out + n);
  }
  // The stages' point_shift (lmx_depth_templates_set_refine_plane): -1 point-to-point, 0..20 point-to-plane against the scene's normals
  // (enableNormals first) with the point term weighted 2^-shift; entry s is stage s of the schedule in force, an empty vector clears it.
  void setRefinePlane(const std::vector<int32_t>& point_shift) {
    check(lmx_depth_templates_set_refine_plane(h_, point_shift.empty() ? nullptr : point_shift.data(), (int32_t)point_shift.size()));
  }
  std::vector<int32_t> refinePlane() const {
    int32_t out[LMX_POSE_MAX_STAGES];
    int32_t n = 0;
    check(lmx_depth_templates_get_refine_plane(h_, out, &n));
    return std::vector<int32_t>(out, out + n);
  }
  // The scene's depth outlier filter ahead of the pose stages (lmx_depth_templates_set_scene_filter, the reference's
  // statisticalOutlierRemoval): sceneFilterDefaults() with the depth frames' camera filled in, or nullptr to turn it off.  struct_size is
  // filled in here.
  static lmx_scene_filter_params sceneFilterDefaults() {
    lmx_scene_filter_params p;
    check(lmx_scene_filter_defaults(&p));
    return p;
  }
  void setSceneFilter(const lmx_scene_filter_params* params) {
    if (!params) { check(lmx_depth_templates_set_scene_filter(h_, nullptr)); return; }
    lmx_scene_filter_params p = *params;
    p.struct_size = (uint32_t)sizeof(lmx_scene_filter_params);
    check(lmx_depth_templates_set_scene_filter(h_, &p));
  }
  // The object's pose in the scene camera from the matched template's view and its refinePoses record (lmx_pose_compose).
  static void composePose(const lmx_mesh_view& view, const lmx_pose_refine_t& refined, double R_obj[9], double t_obj_m[3]) {
    check(lmx_pose_compose(&view, &refined, R_obj, t_obj_m));
  }

  // Pose verification (lmx_pose_verify_matches, the reference's hypothesisVerification stage): out[i] belongs to matches[i] and poses[i],
  // the refinePoses record of the same match.  params.struct_size is filled in here.  With `depth` one frame holding all matches;
  // without, the scene uploadScene left in the object (one frame).
  std::vector<lmx_pose_verify_t> verifyPoses(const std::vector<lmx_match_t>& matches, const std::vector<lmx_pose_refine_t>& poses, lmx_pose_verify_params params,
                                             const Image* depth = nullptr, int class_index = -1) {
    if (poses.size() != matches.size()) throw Exception(LMX_ERR_SHAPE, "DepthTemplates::verifyPoses: one pose per match");
    std::vector<lmx_pose_verify_t> out(matches.size());
    params.struct_size = (uint32_t)sizeof(lmx_pose_verify_params);
    const size_t offsets[2] = {0, matches.size()};
    lmx_image img;
    if (depth) img = depth->c();
    check(lmx_pose_verify_matches(h_, depth ? &img : nullptr, 1, matches.data(), offsets, class_index, poses.data(), &params, out.data()));
    return out;
  }
  std::vector<lmx_pose_verify_t> verifyPoses(const std::vector<lmx_match_t>& matches, const std::vector<lmx_pose_refine_t>& poses, const lmx_pose_verify_params& params,
                                             const Image& depth, int class_index = -1) {
    return verifyPoses(matches, poses, params, &depth, class_index);
  }
  // The parameters with the defaults of the Python front end (the reference's 4 mm voxels); the cameras are the caller's to fill.
  static lmx_pose_verify_params poseVerifyDefaults() {
    lmx_pose_verify_params p = lmx_pose_verify_params();
    p.struct_size = (uint32_t)sizeof(lmx_pose_verify_params);
    p.voxel_mm = 4.0; p.roi_margin = 8;
    return p;
  }
  // The reference's erase rule on verifyPoses records (lmx_pose_verify_keep): kept unless rate < thresh.
  static std::vector<uint8_t> keepVerified(const std::vector<lmx_pose_verify_t>& records, double thresh) {
    std::vector<uint8_t> keep(records.size());
    check(lmx_pose_verify_keep(records.data(), records.size(), thresh, keep.data()));
    return keep;
  }

  // Both stages on the clusters an export left in device memory (lmx_pose_chain_on): per exported cluster the leader match, its
  // refinePoses record, its verifyPoses record and the keepVerified decision, written to the caller's device arrays behind `stream` with
  // no host wait -- what refinePoses / verifyPoses return for the leaders of the same lists, bit for bit.  desc: the export's five arrays
  // and capacities, the five outputs ([cap_clusters] each, chain_header [8]), refine / verify (their struct_size is the caller's to set:
  // poseRefineDefaults(), poseVerifyDefaults()), keep_thresh, class_index or class_base; desc.struct_size and, when 0, desc.n_frames (the
  // frames of the resident scene: 1 unless n_frames says otherwise) are filled in here.  The scene: uploadScene / uploadSceneDevice.
  void poseChain(lmx_pose_chain_desc desc, void* stream = nullptr, int32_t n_frames = 1) {
    desc.struct_size = (uint32_t)sizeof(lmx_pose_chain_desc);
    if (desc.n_frames == 0) desc.n_frames = n_frames;
    check(lmx_pose_chain_on(h_, &desc, stream));
  }

  // The rough pose stage in front of both (lmx_rough_pose_chain_on): per exported cluster the mean view of its largest orientation group,
  // the mesh of `model` (lmx_rough_model_create; the caller's to free) rendered again at that view, that render refined and verified.
  // desc: as poseChain's with rough and member_group in place of leaders and trace_min (lmx_rough_trace_min); the rects of refine and
  // verify stay NULL.
  void roughPoseChain(lmx_rough_model* model, lmx_rough_chain_desc desc, void* stream = nullptr, int32_t n_frames = 1) {
    desc.struct_size = (uint32_t)sizeof(lmx_rough_chain_desc);
    if (desc.n_frames == 0) desc.n_frames = n_frames;
    check(lmx_rough_pose_chain_on(h_, model, &desc, stream));
  }

  // The normal term (lmx_depth_templates_enable_normals): computes and keeps the normals of every crop; needed before normals(),
  // normalDiff() and lmx_ctx_collect_clusters_depth_normal.  fx, fy: the focal lengths of the camera whose depth frames are checked.
  void enableNormals(double fx, double fy, int difference_threshold = 50, int distance_threshold = 2000) {
    const lmx_normal_params p = {fx, fy, difference_threshold, distance_threshold};
    check(lmx_depth_templates_enable_normals(h_, &p));
  }
  // Template id's normals, read back from the device: [h][w][4] int16 = {qx, qy, qz, valid}, a unit normal times 16384.
  std::vector<int16_t> normals(int id) const {
    int32_t r[4] = {0, 0, 0, 0};
    check(lmx_depth_templates_rect(h_, id, r));
    std::vector<int16_t> out((size_t)r[2] * (size_t)r[3] * 4);
    check(lmx_depth_templates_get_normals(h_, id, out.data()));
    return out;
  }
  // diff() with both terms in one pass over each crop: out[i] belongs to matches[i]; ddiffs (may be null) receives what diff() gives.
  std::vector<lmx_normal_diff_t> normalDiff(const std::vector<Image>& depth, const std::vector<lmx_match_t>& matches, const std::vector<size_t>& offsets,
                                            std::vector<lmx_depth_diff_t>* ddiffs = nullptr, int class_index = -1) {
    if (offsets.size() != depth.size() + 1 || offsets.back() != matches.size()) throw Exception(LMX_ERR_SHAPE, "DepthTemplates::normalDiff: offsets must hold one entry per frame plus one and end at matches.size()");
    std::vector<lmx_image> imgs;
    for (const Image& d : depth) imgs.push_back(d.c());
    std::vector<lmx_normal_diff_t> out(matches.size());
    if (ddiffs) ddiffs->resize(matches.size());
    check(lmx_normal_diff_matches(h_, imgs.data(), (int32_t)imgs.size(), matches.data(), offsets.data(), class_index, ddiffs ? ddiffs->data() : nullptr, out.data()));
    return out;
  }
  // The value lmx_ctx_collect_clusters_depth_normal ranks by: minus (mean depth difference in metres + mean normal angle in radians);
  // exp of a cluster's score is the reference's getClusterScore when every member has something to compare.
  static double value(const lmx_depth_diff_t& d, const lmx_normal_diff_t& n, double no_value = -HUGE_VAL) { return lmx_match_value(&d, &n, no_value); }

  // The scene of the next collectClustersDepth: returns without waiting, so call it right after the enqueue.
  void uploadScene(const std::vector<Image>& depth) {
    std::vector<lmx_image> imgs;
    for (const Image& d : depth) imgs.push_back(d.c());
    check(lmx_depth_templates_upload_scene(h_, imgs.data(), (int32_t)imgs.size()));
  }

  // The same for depth frames in device memory (lmx_depth_templates_upload_scene_device): no host frame at all; `stream` as in
  // Detector::uploadDevice.
  void uploadSceneDevice(const std::vector<Image>& depth, void* stream = nullptr) {
    std::vector<lmx_image> imgs;
    for (const Image& d : depth) imgs.push_back(d.c());
    check(lmx_depth_templates_upload_scene_device(h_, imgs.data(), (int32_t)imgs.size(), stream));
  }

  // Moves other's templates behind this object's (lmx_depth_templates_append): other's template i becomes template count() + i, other is
  // left empty.  The classes' objects joined in class order are what Detector::collectClustersClasses scores against.  An object that
  // holds nothing yet becomes an empty one first.
  void append(DepthTemplates& other, int device = 0) {
    if (!h_) check(lmx_depth_templates_from_crops(device, nullptr, nullptr, 0, &h_));
    check(lmx_depth_templates_append(h_, other.h_));
  }

  lmx_depth_templates* handle() const { return h_; }

 private:
  void reset() {
    if (h_) lmx_depth_templates_free(h_);
    h_ = nullptr;
  }
  lmx_depth_templates* h_ = nullptr;
};

inline ClassClusters Detector::collectClustersClasses(const std::vector<std::vector<Image> >& frames, float threshold, DepthTemplates* templates,
                                                      const std::vector<int32_t>& class_base, const std::vector<Image>& depth, bool normals, double no_value,
                                                      size_t capacity) {
  return collect_clusters_classes(frames, threshold, nullptr, templates, class_base, depth, normals, no_value, capacity);
}
inline ClassClusters Detector::collectClustersClasses(const std::vector<std::vector<Image> >& frames, const std::map<std::string, float>& thresholds,
                                                      DepthTemplates* templates, const std::vector<int32_t>& class_base, const std::vector<Image>& depth, bool normals,
                                                      double no_value, size_t capacity) {
  if (thresholds.empty()) throw Exception(LMX_ERR_INVALID_ARG, "collectClustersClasses: an empty threshold map matches no class");
  return collect_clusters_classes(frames, 0.f, &thresholds, templates, class_base, depth, normals, no_value, capacity);
}
inline ClassClusters Detector::collect_clusters_classes(const std::vector<std::vector<Image> >& frames, float threshold, const std::map<std::string, float>* thresholds,
                                                        DepthTemplates* templates, const std::vector<int32_t>& class_base, const std::vector<Image>& depth,
                                                        bool normals, double no_value, size_t capacity) {
  if (frames.empty() || frames[0].empty()) throw Exception(LMX_ERR_SHAPE, "collectClustersClasses: no frames");
  if (templates && (class_base.size() < 2 || depth.size() != frames.size())) throw Exception(LMX_ERR_SHAPE, "collectClustersClasses: class_base needs one entry per class plus one, depth one image per frame");
  const int n = (int)frames.size();
  std::vector<lmx_image> imgs;
  for (const std::vector<Image>& f : frames) {
    if (f.size() != frames[0].size()) throw Exception(LMX_ERR_SHAPE, "collectClustersClasses: every frame needs the same sources");
    for (const Image& s : f) imgs.push_back(s.c());
  }
  ensure_ctx(frames[0][0].cols, frames[0][0].rows, false);
  check(lmx_ctx_upload(ctx_, n, imgs.data(), (int32_t)frames[0].size()));
  if (thresholds) {
    std::vector<std::string> ids;
    const std::vector<float> thr = class_thresholds(*thresholds, &ids);
    std::vector<const char*> cids;
    for (const std::string& c : ids) cids.push_back(c.c_str());
    check(lmx_ctx_enqueue_thresholds(ctx_, n, thr.data(), (int32_t)thr.size(), cids.data(), (int32_t)cids.size()));
  } else {
    check(lmx_ctx_enqueue(ctx_, n, threshold, nullptr, 0));
  }
  ClassClusters out;
  out.matches.resize(capacity); out.clusters.resize(capacity); out.cluster_class.resize(capacity); out.members.resize(capacity);
  out.match_offsets.assign((size_t)n + 1, 0); out.cluster_offsets.assign((size_t)n + 1, 0);
  lmx_class_score score;
  lmx_status st = LMX_OK;
  try {
    if (templates) {
      templates->uploadScene(depth);   // returns at once: the transfer overlaps the match kernels
      out.diffs.resize(capacity);
      if (normals) out.ndiffs.resize(capacity);
      score.templates = templates->handle(); score.class_base = class_base.data(); score.n_classes = (int32_t)class_base.size() - 1;
      score.normals = normals ? 1 : 0; score.no_value = no_value;
    }
    st = lmx_ctx_collect_clusters_classes(ctx_, n, templates ? &score : nullptr, out.matches.data(), capacity, out.match_offsets.data(),
                                          templates ? out.diffs.data() : nullptr, normals ? out.ndiffs.data() : nullptr, out.clusters.data(),
                                          out.cluster_class.data(), capacity, out.cluster_offsets.data(), out.members.data(), capacity);
    check(st);
  } catch (...) {
    // a refusal leaves the enqueue outstanding (an overflow has consumed it): drop it, so that the next call collects its own
    if (st != LMX_ERR_OVERFLOW) (void)lmx_ctx_release(ctx_);
    throw;
  }
  const size_t nm = out.match_offsets[(size_t)n], nc = out.cluster_offsets[(size_t)n];
  size_t nmem = 0;
  for (size_t k = 0; k < nc; ++k) nmem = std::max(nmem, (size_t)out.clusters[k].member_begin + (size_t)out.clusters[k].member_count);
  out.matches.resize(nm); out.clusters.resize(nc); out.cluster_class.resize(nc); out.members.resize(nmem);
  if (templates) out.diffs.resize(nm);
  if (normals) out.ndiffs.resize(nm);
  return out;
}

// The reference's readLinemod (src/rgbdDetector.cpp:1668-1680) with the same shape.
inline std::shared_ptr<Detector> readLinemod(const std::string& filename) {
  std::shared_ptr<Detector> d(new Detector);
  d->read(filename);
  return d;
}

}  // namespace linemod
}  // namespace lmx
