// CPU build of the rough pose stage's shared header (linemod_pose_estimation_amd/csrc/lmx_rough_pose.hpp): runs rp::resolve_slot on lists
// and a view table that tests/rough_pose_cases.py writes to a file, every array on the heap at exactly its stated capacity, so that a
// build with -fsanitize=address,undefined sees any index that leaves an array.
// In:  int32 {n_frames, cap_matches, cap_clusters, cap_members, n_views, class_index, fill, 0}, header[16], frame_info[n_frames][8],
//      matches[cap_matches][5], clusters[cap_clusters][12], members[cap_members]; then doubles: trace_min, views[n_views][10]
//      (R, distance) and D[n_views], ori_dist[n_views].  The quaternions are computed here (rp::quat_of).
// Out: int32 {n_live, header flags}; per slot below n_live int32 {state, flags} and the 152 bytes of its record; member_group[cap_members]
//      (the word `fill` where nothing was written); the quaternions [n_views][4].
// Every slot is decided with 64 lanes and with one; for every slot that has groups, the real std::sort with the reference's comparator
// (group size descending) over the groups must leave the emulation's winner at index 0.
#define LMX_RP_HOST 1
#include "lmx_rough_pose.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace pc = lmx::pc;
namespace rp = lmx::rp;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: rough_pose_host IN OUT\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<unsigned char> bytes;
  unsigned char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
  std::fclose(f);
  size_t at = 0;
  bool short_file = false;
  auto take = [&](size_t n) {
    std::vector<int32_t> out(n);   // exactly n
    if (at + n * 4 > bytes.size()) { short_file = true; return out; }
    if (n) std::memcpy(out.data(), bytes.data() + at, n * 4);
    at += n * 4;
    return out;
  };
  auto take_doubles = [&](size_t n) {
    std::vector<double> out(n);
    if (at + n * 8 > bytes.size()) { short_file = true; return out; }
    if (n) std::memcpy(out.data(), bytes.data() + at, n * 8);
    at += n * 8;
    return out;
  };
  const std::vector<int32_t> head = take(8);
  if (short_file || head[0] < 1 || head[1] < 0 || head[2] < 1 || head[3] < 0 || head[4] < 1) { std::fprintf(stderr, "bad head\n"); return 2; }
  const int32_t n_frames = head[0], n_views = head[4], class_index = head[5], fill = head[6];
  const size_t cap_matches = (size_t)head[1], cap_clusters = (size_t)head[2], cap_members = (size_t)head[3];
  const std::vector<int32_t> header = take(16), info = take((size_t)n_frames * 8), matches = take(cap_matches * 5), clusters = take(cap_clusters * 12),
                             members = take(cap_members);
  const std::vector<double> tm = take_doubles(1), vw = take_doubles((size_t)n_views * 10), D = take_doubles((size_t)n_views), ori = take_doubles((size_t)n_views);
  if (short_file || at != bytes.size()) { std::fprintf(stderr, "the file does not hold what its head announces\n"); return 2; }
  std::vector<pc::Match> m(cap_matches);
  std::vector<pc::Cluster> c(cap_clusters);
  if (cap_matches) std::memcpy(m.data(), matches.data(), cap_matches * sizeof(pc::Match));
  std::memcpy(c.data(), clusters.data(), cap_clusters * sizeof(pc::Cluster));
  std::vector<rp::View> views((size_t)n_views);
  for (int32_t v = 0; v < n_views; ++v) {
    rp::View& t = views[(size_t)v];
    std::memcpy(t.R, &vw[(size_t)v * 10], 9 * sizeof(double));
    t.distance = vw[(size_t)v * 10 + 9]; t.D = D[(size_t)v]; t.ori_dist = ori[(size_t)v];
    rp::quat_of(t.R, t.q);
  }
  const pc::Lists L = {reinterpret_cast<const uint32_t*>(header.data()), info.data(), n_frames, m.data(), c.data(), members.data(), cap_matches, cap_clusters, cap_members};
  const uint32_t live = pc::n_live(L);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  const int32_t top[2] = {(int32_t)live, (int32_t)pc::header_flags(L)};
  std::fwrite(top, 4, 2, o);
  std::vector<int32_t> group(cap_members, fill), group1(cap_members, fill);
  for (uint32_t k = 0; k < live; ++k) {
    rp::Record rec, rec1;
    const rp::Slot s = rp::resolve_slot(L, views.data(), n_views, tm[0], class_index, k, group.data(), &rec);
    const rp::Slot one = rp::resolve_slot(L, views.data(), n_views, tm[0], class_index, k, group1.data(), &rec1, 1);
    if (std::memcmp(&s, &one, sizeof(s)) != 0 || std::memcmp(&rec, &rec1, sizeof(rec)) != 0) { std::fprintf(stderr, "slot %u: 64 lanes and one lane disagree\n", k); return 1; }
    if (s.state == pc::JOB && (rec.status == rp::OK || rec.status == rp::DEGENERATE)) {
      // the reference: std::sort(groups.begin(), groups.end(), by size descending); groups[0]
      std::vector<std::vector<int32_t>> groups((size_t)rec.n_groups);
      for (int32_t p = 0; p < s.member_count; ++p) groups[(size_t)group[(size_t)s.member_begin + (size_t)p]].push_back(p);
      std::vector<const std::vector<int32_t>*> order;
      for (const auto& g : groups) order.push_back(&g);
      std::sort(order.begin(), order.end(), [](const std::vector<int32_t>* a, const std::vector<int32_t>* b) { return a->size() > b->size(); });
      const int32_t win = (int32_t)(order[0] - groups.data());
      if (win != rec.group) { std::fprintf(stderr, "slot %u: std::sort leaves group %d first, the emulation %d\n", k, win, rec.group); return 1; }
    }
    const int32_t st[2] = {s.state, (int32_t)s.flags};
    std::fwrite(st, 4, 2, o);
    std::fwrite(&rec, sizeof(rec), 1, o);
  }
  if (std::memcmp(group.data(), group1.data(), cap_members * 4) != 0) { std::fprintf(stderr, "member_group: 64 lanes and one lane disagree\n"); return 1; }
  if (cap_members) std::fwrite(group.data(), 4, cap_members, o);
  for (const rp::View& t : views) std::fwrite(t.q, sizeof(double), 4, o);
  std::fclose(o);
  return 0;
}
