// Stand-alone driver of expecto_amd/csrc/kmeans_plan.h for tests/test_kmeans_host.py (host compiler
// only, no HIP).  stdin: cases "kind n d ld P" (kind: seed | lloyd) then P rows of 8 integers.
// stdout per case: "error <text>" or "ok k_max t_max u_len idx_len c_len init_len label_len bytes",
// bytes being the workspace of (n, d, k_max, max(t_max, 1), P).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../expecto_amd/csrc/kmeans_plan.h"

int main() {
  char kind[16];
  long long n, d, ld, P;
  while (std::scanf("%15s %lld %lld %lld %lld", kind, &n, &d, &ld, &P) == 5) {
    std::vector<long long> prob((size_t)(P > 0 ? P : 0) * expecto::KM_COLS);
    for (auto& v : prob)
      if (std::scanf("%lld", &v) != 1) return 2;
    expecto::KmeansTotals tot;
    const char* err = expecto::kmeans_check_shape(n, d, ld, P);
    if (!err && P > 0)
      err = std::strcmp(kind, "seed") == 0 ? expecto::kmeans_check_seeding(n, P, prob.data(), &tot)
                                           : expecto::kmeans_check_lloyd(n, P, prob.data(), &tot);
    if (err) {
      std::printf("error %s\n", err);
      continue;
    }
    const long long t = tot.t_max > 0 ? tot.t_max : 1, k = tot.k_max > 0 ? tot.k_max : 1;
    std::printf("ok %lld %lld %lld %lld %lld %lld %lld %lld\n", tot.k_max, tot.t_max, tot.u_len, tot.idx_len, tot.c_len,
                tot.init_len, tot.label_len, expecto::kmeans_workspace_bytes(n, d, k, t, P));
  }
  return 0;
}
