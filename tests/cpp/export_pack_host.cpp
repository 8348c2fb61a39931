// CPU build of csrc/lmx_export_pack.hpp for tests/test_export_pack_host.py: the walks k_export_plan and k_export_pack do with it, one frame
// after the other.  Plain C++: no HIP header, no device.
#include <cstdint>

#include "lmx_export_pack.hpp"

using namespace lmx::xpack;

extern "C" {

// k_export_plan: the frames listed for the large-frame kernel -> large_frames[max_large], returns how many
int32_t xp_plan(const uint32_t* counts, int32_t n_frames, int32_t max_large, uint32_t n_candidates, uint32_t n_records, uint32_t capacity, int32_t* large_frames) {
  int32_t listed = 0;
  if (!list_overflowed(n_candidates, n_records, capacity)) {
    int32_t wanted = 0;
    for (int32_t f = 0; f < n_frames; ++f) {
      const uint32_t* row = counts + (size_t)f * 4;
      const int32_t at = list_index(row, wanted, max_large);
      if (wants_large(row)) ++wanted;
      if (at >= 0) { large_frames[at] = f; listed = at + 1; }
    }
  }
  return listed;
}

// k_export_pack: frame_info[n_frames][8], header[16], and per frame {part, write_matches, write_clusters} in placed[n_frames][3]
void xp_pack(const uint32_t* counts, const uint32_t* lcounts, const uint32_t* raw_records, int32_t n_frames, int32_t max_large, uint32_t n_candidates,
             uint32_t n_records, uint32_t capacity, uint64_t cap_matches, uint64_t cap_clusters, uint64_t cap_members, int32_t* frame_info, uint32_t* header,
             int32_t* placed) {
  const bool overflowed = list_overflowed(n_candidates, n_records, capacity);
  const Caps cap{cap_matches, cap_clusters, cap_members};
  for (int32_t frame = 0; frame < n_frames; ++frame) {   // one workgroup per frame, each redoing the walk up to its own frame
    Walk w;
    Slot s{};
    for (int32_t f = 0; f <= frame; ++f) s = step(w, counts, lcounts, f, max_large, overflowed, cap);
    fill_info(frame_info + (size_t)frame * I_WORDS, s, overflowed ? 0u : raw_records[frame]);
    placed[3 * frame] = s.part; placed[3 * frame + 1] = s.write_matches; placed[3 * frame + 2] = s.write_clusters;
    if (frame == n_frames - 1) fill_header(header, w, n_frames, n_candidates, n_records);
  }
}

}  // extern "C"
