// Stand-alone driver of expecto_amd/csrc/average_linkage.h for tests/test_pwm_cluster_host.py (host
// compiler only, no HIP).  stdin holds cases of two kinds (numbers as hex floats or decimals; "nan" /
// "inf" accepted):
//   "linkage n" then n(n-1)/2 distances
//   "cut n min_cor min_ncor" then 2(n-1) children, n(n-1)/2 cor and n(n-1)/2 ncor
// stdout per case: "case", then "error <text>" or, for a linkage, n-1 lines "merge a b height size" and,
// for a cut, "labels l0 l1 ..." and n-1 lines "mean cor ncor"; then "end".  Floats leave as hex floats.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../expecto_amd/csrc/average_linkage.h"

static bool read_doubles(std::vector<double>& v) {
  char word[64];
  for (double& x : v) {
    if (std::scanf("%63s", word) != 1) return false;
    x = std::strtod(word, nullptr);
  }
  return true;
}

int main() {
  char kind[16];
  int n;
  while (std::scanf("%15s %d", kind, &n) == 2) {
    const long long npair = n >= 2 ? (long long)n * (n - 1) / 2 : 0;
    const size_t m = n >= 2 ? (size_t)n - 1 : 0;
    if (!std::strcmp(kind, "linkage")) {
      std::vector<double> D((size_t)npair), heights(m);
      std::vector<int> children(2 * m), sizes(m);
      if (!read_doubles(D)) return 2;
      std::printf("case\n");
      const int st = expecto::average_linkage(D.data(), n, children.data(), heights.data(), sizes.data());
      if (st != expecto::AVG_OK) {
        std::printf("error %s\n", expecto::average_error_text(st));
      } else {
        for (size_t i = 0; i < m; ++i)
          std::printf("merge %d %d %a %d\n", children[2 * i], children[2 * i + 1], heights[i], sizes[i]);
      }
    } else if (!std::strcmp(kind, "cut")) {
      std::vector<double> thr(2), cor((size_t)npair), ncor((size_t)npair), mean_cor(m), mean_ncor(m);
      std::vector<int> children(2 * m), labels(n >= 2 ? (size_t)n : 0);
      if (!read_doubles(thr)) return 2;
      for (int& c : children)
        if (std::scanf("%d", &c) != 1) return 2;
      if (!read_doubles(cor) || !read_doubles(ncor)) return 2;
      std::printf("case\n");
      const int st = expecto::linkage_threshold_cut(children.data(), n, cor.data(), ncor.data(), thr[0], thr[1],
                                                    labels.data(), mean_cor.data(), mean_ncor.data());
      if (st != expecto::AVG_OK) {
        std::printf("error %s\n", expecto::average_error_text(st));
      } else {
        std::printf("labels");
        for (int l : labels) std::printf(" %d", l);
        std::printf("\n");
        for (size_t i = 0; i < m; ++i) std::printf("mean %a %a\n", mean_cor[i], mean_ncor[i]);
      }
    } else {
      return 3;
    }
    std::printf("end\n");
  }
  return 0;
}
