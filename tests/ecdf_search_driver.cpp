// Stand-alone driver of expecto_amd/csrc/ecdf_search.h for tests/test_ecdf_host.py (host compiler
// only, no HIP).  stdin: cases "K B nq", then the B ascending column values, then the nq queries
// (hex floats or decimals; "nan" / "inf" accepted).  K = 0 stands for the kernel's
// EXPECTO_ECDF_SPLITTERS.  stdout per case: "case", "plan stride m pick_steps finish_steps", one line
// "ge one four" per query -- the count from ecdf_count_ge<1> and from ecdf_count_ge<4> (the kernel's
// width; queries in groups of four, the last group padded with its first query) -- then "end".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../expecto_amd/csrc/ecdf_search.h"
#include "../include/expecto_hip.h"

static bool read_floats(std::vector<float>& out) {
  char word[64];
  for (float& v : out) {
    if (std::scanf("%63s", word) != 1) return false;
    v = std::strtof(word, nullptr);
  }
  return true;
}

int main() {
  int K, B, nq;
  while (std::scanf("%d %d %d", &K, &B, &nq) == 3) {
    if (K == 0) K = EXPECTO_ECDF_SPLITTERS;
    if (K < 1 || B < 1 || nq < 0) return 2;
    std::vector<float> col((size_t)B), q((size_t)nq);
    if (!read_floats(col) || !read_floats(q)) return 2;
    const expecto::EcdfPlan plan = expecto::ecdf_plan(B, K);
    if (plan.m < 1 || plan.m > K) return 3;
    // exactly plan.m splitters and exactly B values: a read past either is the sanitizer's to report
    std::vector<float> spl((size_t)plan.m);
    for (int i = 0; i < plan.m; ++i) spl[(size_t)i] = col[(size_t)expecto::ecdf_splitter_pos(plan, i)];
    std::printf("case\nplan %d %d %d %d\n", plan.stride, plan.m, plan.pick_steps, plan.finish_steps);
    for (int i0 = 0; i0 < nq; i0 += 4) {
      float a4[4];
      int g4[4];
      for (int k = 0; k < 4; ++k) a4[k] = q[(size_t)(i0 + k < nq ? i0 + k : i0)];
      expecto::ecdf_count_ge<4>(col.data(), B, plan, spl.data(), a4, g4);
      for (int k = 0; k < 4 && i0 + k < nq; ++k) {
        const float a1[1] = {a4[k]};
        int g1[1];
        expecto::ecdf_count_ge<1>(col.data(), B, plan, spl.data(), a1, g1);
        std::printf("ge %d %d\n", g1[0], g4[k]);
      }
    }
    std::printf("end\n");
  }
  return 0;
}
