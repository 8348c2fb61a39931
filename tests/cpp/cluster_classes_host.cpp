// lmx_cluster_matches_classes (csrc/lmx_cluster.cpp) as a stand-alone host program, for AddressSanitizer + UBSan: the translation unit is
// compiled into this program with the two functions of the library it calls defined here.  tests/test_cluster_classes_host.py writes the
// cases to a text file (floating-point values as their bit patterns), runs the program on it and compares what it prints with the
// library's answers.
//   file:  n_cases, then per case:  n_matches n_classes has_values
//          n_matches x (x y similarity_bits template_id class_index)   [has_values: n_matches x value_bits]
//          n_classes x (n_templates step radius_min_bits radius_step_bits thresh, n_templates x dist_bits, n_templates x 4 rect)
//   out:   per case and capacity (exact, then 0 / 0):  "status n_clusters", then per cluster that fits
//          "class index[3] rect[4] score_bits member_begin member_count : members..."
#include "lmx_cluster.cpp"

#include <cinttypes>
#include <cstdarg>
#include <cstdio>

static std::string g_error;
namespace lmx {
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}
}  // namespace lmx
extern "C" const char* lmx_last_error(void) { return g_error.c_str(); }

namespace {
bool read_u64(FILE* f, uint64_t* v) { return fscanf(f, "%" SCNu64, v) == 1; }
bool read_i64(FILE* f, long long* v) { return fscanf(f, "%lld", v) == 1; }
double as_double(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }
float as_float(uint64_t b) { const uint32_t w = (uint32_t)b; float x; std::memcpy(&x, &w, 4); return x; }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: cluster_classes_host <cases file>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  long long n_cases = 0;
  if (!read_i64(f, &n_cases)) return 2;
  for (long long k = 0; k < n_cases; ++k) {
    long long n_matches, n_classes, has_values;
    if (!read_i64(f, &n_matches) || !read_i64(f, &n_classes) || !read_i64(f, &has_values)) return 2;
    std::vector<lmx_match_t> m((size_t)n_matches);
    for (lmx_match_t& e : m) {
      long long x, y, t, c;
      uint64_t s;
      if (!read_i64(f, &x) || !read_i64(f, &y) || !read_u64(f, &s) || !read_i64(f, &t) || !read_i64(f, &c)) return 2;
      e.x = (int32_t)x; e.y = (int32_t)y; e.similarity = as_float(s); e.template_id = (int32_t)t; e.class_index = (int32_t)c;
    }
    std::vector<double> values;
    if (has_values)
      for (long long i = 0; i < n_matches; ++i) { uint64_t b; if (!read_u64(f, &b)) return 2; values.push_back(as_double(b)); }
    std::vector<std::vector<double>> dists((size_t)n_classes);
    std::vector<std::vector<int32_t>> rects((size_t)n_classes);
    std::vector<lmx_class_sidecar> classes((size_t)n_classes);
    for (long long c = 0; c < n_classes; ++c) {
      long long nt, step, thresh;
      uint64_t rmin, rstep;
      if (!read_i64(f, &nt) || !read_i64(f, &step) || !read_u64(f, &rmin) || !read_u64(f, &rstep) || !read_i64(f, &thresh)) return 2;
      for (long long i = 0; i < nt; ++i) { uint64_t b; if (!read_u64(f, &b)) return 2; dists[(size_t)c].push_back(as_double(b)); }
      for (long long i = 0; i < 4 * nt; ++i) { long long v; if (!read_i64(f, &v)) return 2; rects[(size_t)c].push_back((int32_t)v); }
      // exact-size heap blocks: the sanitizer sees a read one element past a side-car
      classes[(size_t)c] = lmx_class_sidecar{nt ? dists[(size_t)c].data() : nullptr, nt ? rects[(size_t)c].data() : nullptr, (size_t)nt,
                                             lmx_cluster_params{(int32_t)step, as_double(rmin), as_double(rstep), (int32_t)thresh}};
    }
    for (int pass = 0; pass < 2; ++pass) {
      const size_t cap = pass == 0 ? (size_t)n_matches : 0;
      std::vector<lmx_cluster_t> cl(cap);
      std::vector<int32_t> cls(cap), mem(cap);
      size_t n = 0;
      const lmx_status st = lmx_cluster_matches_classes(m.data(), m.size(), has_values ? values.data() : nullptr, classes.data(), (int32_t)n_classes,
                                                        cap ? cl.data() : nullptr, cap ? cls.data() : nullptr, cap, &n, cap ? mem.data() : nullptr, cap);
      printf("%d %zu\n", (int)st, n);
      if (st != LMX_OK) continue;
      for (size_t i = 0; i < n; ++i) {
        uint64_t bits;
        std::memcpy(&bits, &cl[i].score, 8);
        printf("%d %d %d %d %d %d %d %d %" PRIu64 " %d %d :", cls[i], cl[i].index[0], cl[i].index[1], cl[i].index[2], cl[i].rect[0], cl[i].rect[1], cl[i].rect[2],
               cl[i].rect[3], bits, cl[i].member_begin, cl[i].member_count);
        for (int32_t j = 0; j < cl[i].member_count; ++j) printf(" %d", mem[(size_t)(cl[i].member_begin + j)]);
        printf("\n");
      }
    }
  }
  fclose(f);
  printf("cluster_classes_host ok\n");
  return 0;
}
