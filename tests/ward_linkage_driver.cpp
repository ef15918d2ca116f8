// Stand-alone driver of expecto_amd/csrc/ward_linkage.h for tests/test_ward_host.py (host compiler
// only, no HIP).  stdin: cases "n" then n(n-1)/2 distances (hex floats or decimals; "nan" / "inf"
// accepted).  stdout per case: "case", then "error <text>" or n-1 lines "merge a b height size" with
// the height as a hex float, then "end".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../expecto_amd/csrc/ward_linkage.h"

int main() {
  int n;
  while (std::scanf("%d", &n) == 1) {
    const long long npair = n >= 2 ? (long long)n * (n - 1) / 2 : 0;
    std::vector<double> D((size_t)npair);
    char word[64];
    for (long long p = 0; p < npair; ++p) {
      if (std::scanf("%63s", word) != 1) return 2;
      D[(size_t)p] = std::strtod(word, nullptr);
    }
    const size_t m = n >= 2 ? (size_t)n - 1 : 0;
    std::vector<int> children(2 * m), sizes(m);
    std::vector<double> heights(m);
    std::printf("case\n");
    const int st = expecto::ward_linkage(D.data(), n, children.data(), heights.data(), sizes.data());
    if (st != expecto::WARD_OK) {
      std::printf("error %s\n", expecto::ward_error_text(st));
    } else {
      for (size_t i = 0; i < m; ++i)
        std::printf("merge %d %d %a %d\n", children[2 * i], children[2 * i + 1], heights[i], sizes[i]);
    }
    std::printf("end\n");
  }
  return 0;
}
