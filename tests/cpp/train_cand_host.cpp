// The mesh trainer's candidate lists on the CPU (linemod_pose_estimation_amd/csrc/lmx_train_cand.hpp: the header the kernel k_train_candidates
// is written with, compiled here without HIP) and the host's rank-and-select on such a list (lmx_train_select.hpp: select_from_list), behind a
// C interface.  Compiled with g++ by tests/test_train_cand_host.py and tests/test_gpu_train_candidates.py and, under
// -fsanitize=address,undefined, into tests/cpp/train_cand_main.cpp.  Every array is copied into a vector of exactly its size first.
//   tch_window : one window (the whole image) -> its list: records [n][2] words {x | y << 14 | label << 28, float score}, header[16]
//   tch_select : a list -> the selected features (window coordinates)
#include <cstring>
#include <string>
#include <vector>

#include "lmx_train_select.hpp"

namespace ts = lmx::train_select;
namespace tc = lmx::train_cand;

extern "C" {

// -> the number of candidates (records filled, header filled), -1: the window is too large for the device path, -2: more than cap candidates
int tch_window(int color, const uint8_t* label, const float* mag, const uint8_t* mask, int H, int W, float strong_threshold, int extract_threshold,
               uint32_t* records, int cap, uint32_t* header) {
  const size_t n = (size_t)H * W;
  const std::vector<uint8_t> lab(label, label + n), msk(mask ? mask : label, mask ? mask + n : label);
  tc::WindowList out;
  if (color) {
    const std::vector<float> mg(mag, mag + n);
    tc::color_window(lab.data(), mg.data(), mask ? msk.data() : nullptr, H, W, strong_threshold, &out);
  } else {
    tc::depth_window(lab.data(), mask ? msk.data() : nullptr, H, W, extract_threshold, &out);
  }
  std::memcpy(header, &out.header, sizeof(out.header));
  if (out.header.status == tc::ST_TOO_LARGE) return -1;
  if (out.records.size() > (size_t)cap) return -2;
  if (!out.records.empty()) std::memcpy(records, out.records.data(), out.records.size() * sizeof(tc::Record));
  return (int)out.records.size();
}

// -> feature count (== num_features), -1 rejected, -2 refused (num_features outside 1 .. 63)
int tch_select(int color, const uint32_t* records, const uint32_t* header, int num_features, int32_t* feats) {
  std::string why;
  if (!ts::check_num_features({ts::Modality{color != 0, num_features, 0.0f, 0}}, 1, &why)) return -2;
  tc::ListHeader hd;
  std::memcpy(&hd, header, sizeof(hd));
  std::vector<tc::Record> recs(hd.n_cands);
  if (hd.n_cands) std::memcpy(recs.data(), records, recs.size() * sizeof(tc::Record));
  std::vector<ts::Feat> out;
  if (!ts::select_from_list(color != 0, hd, recs.data(), 0, 0, (size_t)num_features, out)) return -1;
  for (size_t i = 0; i < out.size(); ++i) { feats[3 * i] = out[i].x; feats[3 * i + 1] = out[i].y; feats[3 * i + 2] = out[i].label; }
  return (int)out.size();
}

}  // extern "C"
