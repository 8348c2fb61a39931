// CPU build of what csrc/lmx_export_pack.hpp adds for lmx_ctx_export_clusters_on, for tests/test_export_clusters_pack_host.py: k_export_pack's
// walk, one frame after the other, and per frame where diffs, ndiffs and cluster_class go and whether they are written.  Plain C++: no HIP
// header, no device.
#include <cstdint>

#include "lmx_export_pack.hpp"

using namespace lmx::xpack;

extern "C" {

// side[n_frames][8] = {diff_begin, n_diffs, write_diffs, write_ndiffs, class_begin, n_class, write_cluster_class, status};
// `has` = bit 0 diffs, bit 1 ndiffs, bit 2 cluster_class
void xpc_side(const uint32_t* counts, const uint32_t* lcounts, int32_t n_frames, int32_t max_large, uint32_t n_candidates, uint32_t n_records,
              uint32_t capacity, uint64_t cap_matches, uint64_t cap_clusters, uint64_t cap_members, int32_t has, int64_t* side) {
  const bool overflowed = list_overflowed(n_candidates, n_records, capacity);
  const Caps cap{cap_matches, cap_clusters, cap_members};
  const SideArrays arrays{(has & 1) != 0, (has & 2) != 0, (has & 4) != 0};
  for (int32_t frame = 0; frame < n_frames; ++frame) {
    Walk w;
    Slot s{};
    for (int32_t f = 0; f <= frame; ++f) s = step(w, counts, lcounts, f, max_large, overflowed, cap);
    const SideSlot o = side_slot(s, arrays);
    int64_t* row = side + (size_t)frame * 8;
    row[0] = (int64_t)o.diff_begin; row[1] = o.n_diffs; row[2] = o.write_diffs; row[3] = o.write_ndiffs;
    row[4] = (int64_t)o.class_begin; row[5] = o.n_class; row[6] = o.write_cluster_class; row[7] = s.status;
  }
}

uint32_t xpc_diff_dwords() { return kDiffDwords; }

}  // extern "C"
