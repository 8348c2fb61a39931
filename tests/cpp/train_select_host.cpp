// The trainer's host half (linemod_pose_estimation_amd/csrc/lmx_train_select.hpp: plain C++, no HIP) behind a C interface, compiled with g++
// by tests/test_train_select_host.py and, under -fsanitize=address,undefined, into tests/cpp/train_select_main.cpp.  Every array is copied
// into a vector of exactly its size before the header sees it, so that a sanitizer build sees any read outside a level image or a window.
//   tsh_extract : extract_color / extract_depth on one whole image, the features as selected (image coordinates)
//   tsh_pyramid : mode 0 = extract_* on whole frames + crop_templates, the way upstream runs;  mode 1 = select_pyramid, what both trainers
//                 call (window rule inside);  arrays may be packed windows at (x0[l], y0[l]) of their level (the mesh trainer's form)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lmx_train_select.hpp"

namespace ts = lmx::train_select;

extern "C" {

// -> feature count (== num_features), -1 rejected, -2 refused (num_features outside 1 .. 63)
int tsh_extract(int color, const uint8_t* label, const float* mag, const uint8_t* mask, int H, int W, int num_features, float strong_threshold,
                int extract_threshold, int32_t* feats) {
  std::string why;
  if (!ts::check_num_features({ts::Modality{color != 0, num_features, strong_threshold, extract_threshold}}, 1, &why)) return -2;
  const size_t n = (size_t)H * W;
  const std::vector<uint8_t> lab(label, label + n), msk(mask ? mask : label, mask ? mask + n : label);
  std::vector<ts::Feat> out;
  bool ok;
  if (color) ok = ts::extract_color(lab, std::vector<float>(mag, mag + n), msk, H, W, (size_t)num_features, strong_threshold, out);
  else ok = ts::extract_depth(lab, msk, H, W, (size_t)num_features, extract_threshold, out);
  if (!ok) return -1;
  for (size_t i = 0; i < out.size(); ++i) { feats[3 * i] = out[i].x; feats[3 * i + 1] = out[i].y; feats[3 * i + 2] = out[i].label; }
  return (int)out.size();
}

// -> 0 accepted (templates [L*M][5], features [n][3], bb[4] filled), 1 rejected, 2 refused (the reason in err)
int tsh_pyramid(int mode, int n_levels, int n_mod, const int* is_color, const int* rows, const int* cols, const int* x0, const int* y0,
                const void* const* label, const void* const* mag, const void* const* mask, const int* num_features, const float* strong_threshold,
                const int* extract_threshold, int32_t* templates, int32_t* features, int32_t* bb, char* err, int err_len) {
  std::vector<ts::Modality> mods;
  for (int m = 0; m < n_mod; ++m) mods.push_back(ts::Modality{is_color[m] != 0, num_features[m], strong_threshold[m], extract_threshold[m]});
  // exact-size copies
  std::vector<std::vector<uint8_t>> labs((size_t)n_levels * n_mod), msks(n_levels);
  std::vector<std::vector<float>> mags((size_t)n_levels * n_mod);
  std::vector<ts::LevelArrays> levels(n_levels);
  for (int l = 0; l < n_levels; ++l) {
    const size_t n = (size_t)rows[l] * cols[l];
    ts::LevelArrays& lv = levels[l];
    lv.w = cols[l]; lv.h = rows[l]; lv.x0 = x0 ? x0[l] : 0; lv.y0 = y0 ? y0[l] : 0;
    for (int m = 0; m < n_mod; ++m) {
      const size_t k = (size_t)l * n_mod + m;
      labs[k].assign((const uint8_t*)label[k], (const uint8_t*)label[k] + n);
      lv.label.push_back(labs[k].data());
      if (is_color[m]) mags[k].assign((const float*)mag[k], (const float*)mag[k] + n);
      lv.mag.push_back(is_color[m] ? mags[k].data() : nullptr);
    }
    if (mask[l]) { msks[l].assign((const uint8_t*)mask[l], (const uint8_t*)mask[l] + n); lv.mask = msks[l].data(); }
  }
  ts::Pyramid pyr;
  std::string why;
  ts::Status st = ts::ACCEPTED;
  if (mode == 1) {
    st = ts::select_pyramid(levels, mods, &pyr, &why);
  } else {
    if (!ts::check_num_features(mods, n_levels, &why)) st = ts::BAD_ARGUMENT;
    std::vector<std::vector<ts::Feat>> tp((size_t)n_levels * n_mod);
    for (int m = 0; m < n_mod && st == ts::ACCEPTED; ++m) {
      size_t nf = (size_t)mods[m].num_features;
      int et = mods[m].extract_threshold;
      for (int l = 0; l < n_levels && st == ts::ACCEPTED; ++l) {
        if (l > 0) { nf /= 2; et /= 2; }
        const size_t k = (size_t)l * n_mod + m;
        const bool ok = mods[m].color ? ts::extract_color(labs[k], mags[k], msks[l], rows[l], cols[l], nf, mods[m].strong_threshold, tp[k])
                                      : ts::extract_depth(labs[k], msks[l], rows[l], cols[l], nf, et, tp[k]);
        if (!ok) st = ts::REJECTED;
        for (ts::Feat& f : tp[k]) { f.x += levels[l].x0; f.y += levels[l].y0; }
      }
    }
    if (st == ts::ACCEPTED) ts::crop_templates(tp, n_mod, &pyr);
  }
  if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", why.c_str());
  if (st != ts::ACCEPTED) return (int)st;
  std::memcpy(templates, pyr.templates.data(), pyr.templates.size() * sizeof(int32_t));
  std::memcpy(features, pyr.features.data(), pyr.features.size() * sizeof(int32_t));
  std::memcpy(bb, pyr.bounding_box, sizeof(pyr.bounding_box));
  return 0;
}

}  // extern "C"
