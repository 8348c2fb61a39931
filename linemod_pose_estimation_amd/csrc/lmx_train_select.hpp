// Host half of the trainer: extractTemplate's candidate ranking, the greedy scattered selection and cropTemplates of
// cv::linemod, on label / magnitude / mask arrays that the device half produced.  No HIP here and no lmx_internal.hpp: plain C++ that
// lmx_train.cpp includes and that tests/cpp/train_select_host.cpp compiles with g++, so tests/test_train_select_host.py checks it against
// the oracle on the CPU.  select_pyramid() is the one form of "per-level window, crop, extract, shift back, cropTemplates"; both trainers
// (train_add_template on whole frames, select_view on the packed windows of the mesh trainer) only collect the arrays and call it.
// The mesh trainer's device path delivers each window's candidate list instead of arrays (lmx_train_cand.hpp, which compiles as plain C++
// too): select_from_list decodes it and runs rank_select_color / rank_select_depth, the sequential rest the two extract functions end in.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <stdexcept>
#include <vector>

#include "lmx_train_cand.hpp"

namespace lmx {
namespace train_select {

struct Cand { int x, y, label; float score; };
struct Feat { int x, y, label; };

inline int label_of(uint8_t q) {  // upstream getLabel(): one-hot byte -> bin
  for (int k = 0; k < 8; ++k)
    if (q == (1u << k)) return k;
  return -1;
}

// 3x3 minimum with BORDER_REPLICATE (cv::erode with the default 3x3 rectangle)
inline std::vector<uint8_t> erode3(const std::vector<uint8_t>& m, int H, int W) {
  std::vector<uint8_t> out((size_t)H * W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint8_t v = 255;
      for (int dy = -1; dy <= 1; ++dy) {
        const int yy = std::min(std::max(y + dy, 0), H - 1);
        for (int dx = -1; dx <= 1; ++dx) v = std::min(v, m[(size_t)yy * W + std::min(std::max(x + dx, 0), W - 1)]);
      }
      out[(size_t)y * W + x] = v;
    }
  return out;
}

// distanceTransform(src, dst, DIST_C, 3): chessboard distance to the nearest zero pixel (two-pass 8-neighbour chamfer with unit
// weights, exact for that metric); a component without any zero pixel in the image keeps a huge value, like upstream's
// initial distance.
inline std::vector<float> dist_chessboard(const std::vector<uint8_t>& nz, int H, int W) {
  const int INF = 1 << 28;
  std::vector<int> d((size_t)H * W);
  for (size_t i = 0; i < d.size(); ++i) d[i] = nz[i] ? INF : 0;
  auto at = [&](int y, int x) -> int { return (y < 0 || y >= H || x < 0 || x >= W) ? INF : d[(size_t)y * W + x]; };
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int v = d[(size_t)y * W + x];
      v = std::min(v, std::min(std::min(at(y - 1, x - 1), at(y - 1, x)), std::min(at(y - 1, x + 1), at(y, x - 1))) + 1);
      d[(size_t)y * W + x] = v;
    }
  for (int y = H - 1; y >= 0; --y)
    for (int x = W - 1; x >= 0; --x) {
      int v = d[(size_t)y * W + x];
      v = std::min(v, std::min(std::min(at(y + 1, x + 1), at(y + 1, x)), std::min(at(y + 1, x - 1), at(y, x + 1))) + 1);
      d[(size_t)y * W + x] = v;
    }
  std::vector<float> out(d.size());
  for (size_t i = 0; i < d.size(); ++i) out[i] = (float)d[i];
  return out;
}

// QuantizedPyramid::selectScatteredFeatures
inline void select_scattered(const std::vector<Cand>& cands, std::vector<Feat>& feats, size_t num_features, float distance) {
  feats.clear();
  float distance_sq = distance * distance;
  int i = 0;
  while (feats.size() < num_features) {
    const Cand& c = cands[i];
    bool keep = true;
    for (size_t j = 0; j < feats.size() && keep; ++j) {
      const int dx = c.x - feats[j].x, dy = c.y - feats[j].y;
      keep = (float)(dx * dx + dy * dy) >= distance_sq;
    }
    if (keep) feats.push_back(Feat{c.x, c.y, c.label});
    if (++i == (int)cands.size()) {
      i = 0;
      distance -= 1.0f;
      distance_sq = distance * distance;
    }
  }
}

inline bool by_score_desc(const Cand& a, const Cand& b) { return a.score > b.score; }  // Candidate::operator<

// The sequential rest of the two extractTemplates, on a candidate list in raster order: extract_color / extract_depth below collect the list
// from images; the mesh trainer's device path (lmx_train_cand.hpp) delivers it ready-made.  `cands` is reordered (and, for DepthNormal,
// its raw distances divided by the label counts).  false: fewer candidates than features, the template is rejected.
inline bool rank_select_color(std::vector<Cand>& cands, size_t num_features, std::vector<Feat>& out) {
  if (cands.size() < num_features) return false;
  std::stable_sort(cands.begin(), cands.end(), by_score_desc);
  const float distance = static_cast<float>(cands.size() / num_features + 1);
  select_scattered(cands, out, num_features, distance);
  return true;
}
inline bool rank_select_depth(std::vector<Cand>& cands, const int label_counts[8], size_t area, size_t num_features, std::vector<Feat>& out) {
  if (cands.size() < num_features) return false;
  for (Cand& c : cands) c.score /= (float)label_counts[c.label];
  std::stable_sort(cands.begin(), cands.end(), by_score_desc);
  const float distance = sqrtf((float)area) / sqrtf((float)num_features) + 1.5f;
  select_scattered(cands, out, num_features, distance);
  return true;
}

// One window's candidate list as the device path delivers it (lmx_train_cand.hpp) -> the selected features, shifted by the window's origin
// (x0, y0) into level coordinates.  false: rejected.
inline bool select_from_list(bool color, const train_cand::ListHeader& hd, const train_cand::Record* recs, int x0, int y0, size_t num_features,
                             std::vector<Feat>& out) {
  std::vector<Cand> cands(hd.n_cands);
  for (size_t i = 0; i < cands.size(); ++i) {
    const int label = train_cand::rec_label(recs[i].xyl);
    if (!color && label < 0) throw std::runtime_error("candidate list holds a DepthNormal record without a label");
    cands[i] = Cand{train_cand::rec_x(recs[i].xyl) + x0, train_cand::rec_y(recs[i].xyl) + y0, label, recs[i].score};
  }
  if (color) return rank_select_color(cands, num_features, out);
  int label_counts[8];
  for (int k = 0; k < 8; ++k) label_counts[k] = (int)hd.label_counts[k];
  return rank_select_depth(cands, label_counts, (size_t)hd.area, num_features, out);
}

// ColorGradientPyramid::extractTemplate
inline bool extract_color(const std::vector<uint8_t>& angle, const std::vector<float>& mag, const std::vector<uint8_t>& mask, int H, int W,
                          size_t num_features, float strong_threshold, std::vector<Feat>& out) {
  std::vector<uint8_t> local;
  const bool no_mask = mask.empty();
  if (!no_mask) {
    std::vector<uint8_t> er = erode3(mask, H, W);
    local.resize(mask.size());
    for (size_t i = 0; i < mask.size(); ++i) local[i] = (uint8_t)(mask[i] > er[i] ? mask[i] - er[i] : 0);  // subtract saturates
  }
  const float threshold_sq = strong_threshold * strong_threshold;
  std::vector<Cand> cands;
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const size_t i = (size_t)r * W + c;
      if (!no_mask && !local[i]) continue;
      const uint8_t q = angle[i];
      if (q > 0 && mag[i] > threshold_sq) cands.push_back(Cand{c, r, label_of(q), mag[i]});
    }
  return rank_select_color(cands, num_features, out);
}

// DepthNormalPyramid::extractTemplate
inline bool extract_depth(const std::vector<uint8_t>& normal, const std::vector<uint8_t>& mask, int H, int W, size_t num_features,
                          int extract_threshold, std::vector<Feat>& out) {
  std::vector<uint8_t> local;
  const bool no_mask = mask.empty();
  if (!no_mask) local = erode3(erode3(mask, H, W), H, W);  // erode(..., iterations = 2, BORDER_REPLICATE)
  std::vector<float> dist[8];
  std::vector<uint8_t> temp((size_t)H * W);
  for (int k = 0; k < 8; ++k) {
    for (size_t i = 0; i < temp.size(); ++i) temp[i] = (uint8_t)(((no_mask || local[i]) ? (1u << k) : 0u) & normal[i]);
    dist[k] = dist_chessboard(temp, H, W);
  }
  int label_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<Cand> cands;
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const size_t i = (size_t)r * W + c;
      if (!no_mask && !local[i]) continue;
      const uint8_t q = normal[i];
      if (q == 0 || q == 255) continue;
      const int label = label_of(q);
      if (label < 0) continue;
      const float score = dist[label][i];
      if (score >= (float)extract_threshold) {
        cands.push_back(Cand{c, r, label, score});
        ++label_counts[label];
      }
    }
  size_t area = normal.size();
  if (!no_mask) { area = 0; for (uint8_t v : local) area += v != 0; }
  return rank_select_depth(cands, label_counts, area, num_features, out);
}

// The window rule.  With an object mask (what the reference's trainers pass: the rendered silhouette) everything extractTemplate looks at
// lies inside the mask's bounding box: candidates exist only where the eroded mask is set, and the erosions and the chessboard distance
// transforms at those pixels depend only on pixels within 2 of the box (outside the mask every intermediate image is zero).  The stages
// therefore run on the box grown by 2 pixels (clamped to the image, where BORDER_REPLICATE keeps its meaning) instead of the whole
// frame -- the same values, the same candidate order (raster order is preserved), 10-20x fewer pixels for a rendered object: eight
// full-frame distance transforms were most of the 16 ms a 640x480 RGB-D view took (round 3).
struct Win { int x0, y0, w, h; };
inline Win mask_window(const uint8_t* mask /* null: no mask */, int w, int h) {
  Win win{0, 0, w, h};
  if (!mask) return win;
  int bx0 = w, by0 = h, bx1 = -1, by1 = -1;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      if (mask[(size_t)y * w + x]) { bx0 = std::min(bx0, x); bx1 = std::max(bx1, x); by0 = std::min(by0, y); by1 = std::max(by1, y); }
  if (bx1 >= 0) {
    win.x0 = std::max(0, bx0 - 2); win.y0 = std::max(0, by0 - 2);
    win.w = std::min(w, bx1 + 3) - win.x0; win.h = std::min(h, by1 + 3) - win.y0;
  } else {
    win = Win{0, 0, std::min(w, 4), std::min(h, 4)};   // an all-zero mask: no candidates anywhere, any window shows that
  }
  return win;
}

// What a modality contributes to the selection (lmx_modality_desc without the quantiser's thresholds)
struct Modality {
  bool color;              // ColorGradient (labels + squared magnitudes) or DepthNormal (labels)
  int num_features;        // at level 0; halved per level like upstream's pyrDown
  float strong_threshold;  // ColorGradient
  int extract_threshold;   // DepthNormal, at level 0; halved per level
};

// One pyramid level's arrays, packed w x h: either the whole level image (x0 = y0 = 0) or a window of it whose top-left pixel is
// (x0, y0) in the level image and that holds the mask's box grown by 2 (mesh_window).
struct LevelArrays {
  int w = 0, h = 0, x0 = 0, y0 = 0;
  std::vector<const uint8_t*> label;   // [M]
  std::vector<const float*> mag;       // [M], null for DepthNormal
  const uint8_t* mask = nullptr;       // null: no object mask
};

struct Pyramid {
  std::vector<int32_t> templates;   // [L*M][5] {width, height, level, feat_begin, feat_count}, template k = l * M + m
  std::vector<int32_t> features;    // [n][3] {x, y, label}, relative to the bounding box
  int32_t bounding_box[4] = {0, 0, 0, 0};
};

enum Status { ACCEPTED = 0, REJECTED = 1, BAD_ARGUMENT = 2 };

// Every level's feature count must lie in 1 .. 63: a count halved to 0 would divide by zero in extractTemplate (upstream does), one
// above 63 does not fit the device tables.  Returns false with the reason in *error.
inline bool check_num_features(const std::vector<Modality>& mods, int n_levels, std::string* error) {
  for (size_t m = 0; m < mods.size(); ++m) {
    int nf = mods[m].num_features;
    for (int l = 0; l < n_levels; ++l) {
      if (l > 0) nf /= 2;
      if (nf < 1 || nf > 63) {
        if (error)
          *error = nf < 1 ? "modality " + std::to_string(m) + ": num_features " + std::to_string(mods[m].num_features) + " leaves " + std::to_string(nf) +
                                " features at pyramid level " + std::to_string(l) + " (at least 1 is needed at every level)"
                          : "num_features " + std::to_string(nf) + " > 63";
        return false;
      }
    }
  }
  return true;
}

// cropTemplates: tp[k = l * M + m] holds level-l image coordinates
inline void crop_templates(const std::vector<std::vector<Feat>>& tp, int n_mod, Pyramid* out) {
  const int n = (int)tp.size();
  int min_x = INT32_MAX, min_y = INT32_MAX, max_x = INT32_MIN, max_y = INT32_MIN;
  for (int k = 0; k < n; ++k) {
    const int level = k / n_mod;
    for (const Feat& f : tp[k]) {
      const int x = f.x << level, y = f.y << level;
      min_x = std::min(min_x, x); min_y = std::min(min_y, y); max_x = std::max(max_x, x); max_y = std::max(max_y, y);
    }
  }
  if (min_x % 2 == 1) --min_x;
  if (min_y % 2 == 1) --min_y;
  out->templates.clear(); out->features.clear();
  int32_t fb = 0;
  for (int k = 0; k < n; ++k) {
    const int level = k / n_mod;
    const int ox = min_x >> level, oy = min_y >> level;
    out->templates.insert(out->templates.end(), {(max_x - min_x) >> level, (max_y - min_y) >> level, level, fb, (int32_t)tp[k].size()});
    for (const Feat& f : tp[k]) out->features.insert(out->features.end(), {f.x - ox, f.y - oy, f.label});
    fb += (int32_t)tp[k].size();
  }
  out->bounding_box[0] = min_x; out->bounding_box[1] = min_y; out->bounding_box[2] = max_x - min_x; out->bounding_box[3] = max_y - min_y;
}

// extractTemplate per (modality, level) on the window of each level, then cropTemplates: Detector::addTemplate after the per-pixel stages.
// REJECTED: some level yields too few candidates (upstream: addTemplate returns -1, nothing is added).
inline Status select_pyramid(const std::vector<LevelArrays>& levels, const std::vector<Modality>& mods, Pyramid* out, std::string* error) {
  const int L = (int)levels.size(), M = (int)mods.size();
  if (!check_num_features(mods, L, error)) return BAD_ARGUMENT;
  std::vector<Win> wins(L);
  for (int l = 0; l < L; ++l) wins[l] = mask_window(levels[l].mask, levels[l].w, levels[l].h);
  std::vector<std::vector<Feat>> tp((size_t)L * M);
  for (int m = 0; m < M; ++m) {
    const Modality& md = mods[m];
    size_t num_features = (size_t)md.num_features;
    int extract_threshold = md.extract_threshold;
    for (int l = 0; l < L; ++l) {
      if (l > 0) { num_features /= 2; extract_threshold /= 2; }
      const LevelArrays& lv = levels[l];
      const Win& win = wins[l];
      const size_t n = (size_t)win.w * win.h;
      std::vector<uint8_t> lab(n), msk(lv.mask ? n : 0);
      for (int y = 0; y < win.h; ++y) {
        std::memcpy(&lab[(size_t)y * win.w], lv.label[m] + (size_t)(win.y0 + y) * lv.w + win.x0, (size_t)win.w);
        if (lv.mask) std::memcpy(&msk[(size_t)y * win.w], lv.mask + (size_t)(win.y0 + y) * lv.w + win.x0, (size_t)win.w);
      }
      std::vector<Feat>& f = tp[(size_t)l * M + m];
      bool ok;
      if (md.color) {
        std::vector<float> mg(n);
        for (int y = 0; y < win.h; ++y) std::memcpy(&mg[(size_t)y * win.w], lv.mag[m] + (size_t)(win.y0 + y) * lv.w + win.x0, (size_t)win.w * sizeof(float));
        ok = extract_color(lab, mg, msk, win.h, win.w, num_features, md.strong_threshold, f);
      } else {
        ok = extract_depth(lab, msk, win.h, win.w, num_features, extract_threshold, f);
      }
      if (!ok) return REJECTED;
      for (Feat& ft : f) { ft.x += win.x0 + lv.x0; ft.y += win.y0 + lv.y0; }
    }
  }
  crop_templates(tp, M, out);
  return ACCEPTED;
}

}  // namespace train_select
}  // namespace lmx
