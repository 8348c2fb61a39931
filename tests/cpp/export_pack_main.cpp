// Stand-alone run of csrc/lmx_export_pack.hpp for sanitizer builds (tests/test_export_pack_host.py): every table of a case file in heap
// blocks of exactly the size the kernels are given, so that an index past a count row, a list or frame_info ends the program.
//   export_pack_main <cases.u32>
// file: n_cases, then per case {n_frames, max_large, n_candidates, n_records, capacity, cap_matches, cap_clusters, cap_members,
// counts[n_frames][4], lcounts[max(1, max_large)][4], raw_records[n_frames]} as uint32.  Prints per case one line: the listed frames |
// frame_info | header | placed.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "export_pack_host.cpp"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: export_pack_main cases.u32\n"); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
  const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const uint32_t* w = reinterpret_cast<const uint32_t*>(raw.data());
  const uint32_t* const end = w + raw.size() / 4;
  const uint32_t n_cases = *w++;
  for (uint32_t c = 0; c < n_cases; ++c) {
    if (end - w < 8) return 3;
    const int32_t F = (int32_t)w[0], max_large = (int32_t)w[1];
    const uint32_t n_cand = w[2], n_rec = w[3], capacity = w[4];
    const uint64_t caps[3] = {w[5], w[6], w[7]};
    w += 8;
    const size_t n_l = (size_t)(max_large > 0 ? max_large : 1);
    if ((size_t)(end - w) < (size_t)F * 5 + n_l * 4) return 3;
    const std::vector<uint32_t> counts(w, w + (size_t)F * 4), lcounts(w + (size_t)F * 4, w + (size_t)F * 4 + n_l * 4),
        records(w + (size_t)F * 4 + n_l * 4, w + (size_t)F * 5 + n_l * 4);
    w += (size_t)F * 5 + n_l * 4;
    std::vector<int32_t> list(n_l, -1), info((size_t)F * 8), placed((size_t)F * 3);
    std::vector<uint32_t> header(16);
    const int32_t listed = xp_plan(counts.data(), F, max_large, n_cand, n_rec, capacity, list.data());
    xp_pack(counts.data(), lcounts.data(), records.data(), F, max_large, n_cand, n_rec, capacity, caps[0], caps[1], caps[2], info.data(), header.data(), placed.data());
    for (int32_t i = 0; i < listed; ++i) std::printf("%d ", list[(size_t)i]);
    std::printf("|");
    for (int32_t v : info) std::printf(" %d", v);
    std::printf(" |");
    for (uint32_t v : header) std::printf(" %u", v);
    std::printf(" |");
    for (int32_t v : placed) std::printf(" %d", v);
    std::printf("\n");
  }
  std::printf("export_pack_main ok %u cases\n", n_cases);
  return 0;
}
