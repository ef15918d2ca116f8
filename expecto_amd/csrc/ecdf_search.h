// The search arithmetic of expecto_ecdf_tail_counts (ecdf.hip), as plain C++ with no HIP types: it
// compiles with the host compiler alone (tests/ecdf_search_driver.cpp) and, with ECDF_HD defined
// as __host__ __device__, inside the kernel.
//
// A column holds B values sorted ascending.  lb(a) = #{b : col[b] < a} is found in two levels:
//   plan      stride = ceil(B / K), m = ceil(B / stride) <= K splitters, splitter i = col[i * stride];
//             B <= K gives stride 1: the splitters are the column and the second level is empty;
//   pick      p = #{i < m : splitter[i] < a}, a lower bound over the splitters;
//   range     p == 0: lb = 0.  Else col[(p-1)*stride] < a, and col[p*stride] >= a where p < m, so
//             lb lies in [(p-1)*stride + 1, min(p*stride, B)]: at most stride - 1 candidates;
//   finish    a lower bound over col[lo .. hi).
// Both lower bounds run a fixed number of halving steps (ecdf_steps of the largest candidate
// count), N queries side by side, so a wave never diverges and every step issues N independent
// loads; a query whose range is already empty reads element 0 (always there, B >= 1) and keeps
// its range.  A NaN query compares false everywhere (lb = 0); the caller gives it ge = -1.
#pragma once

#ifndef ECDF_HD
#define ECDF_HD
#endif

namespace expecto {

struct EcdfPlan {
  int stride;        // distance of two splitters in the column
  int m;             // splitters per column, 1 .. K
  int pick_steps;    // halving steps of the lower bound over m splitters
  int finish_steps;  // halving steps of the lower bound over stride - 1 candidates
};

// Halving steps that empty a range of c candidates: the bit length of c.
ECDF_HD inline int ecdf_steps(int c) {
  int s = 0;
  while (c > 0) {
    c >>= 1;
    ++s;
  }
  return s;
}

// 1 <= B <= 2^31 - 2, K >= 1.
ECDF_HD inline EcdfPlan ecdf_plan(int B, int K) {
  EcdfPlan p;
  p.stride = (int)(((long long)B + K - 1) / K);
  p.m = (int)(((long long)B + p.stride - 1) / p.stride);
  p.pick_steps = ecdf_steps(p.m);
  p.finish_steps = ecdf_steps(p.stride - 1);
  return p;
}

// Position in the column of splitter i (i < m).
ECDF_HD inline long long ecdf_splitter_pos(const EcdfPlan& plan, int i) { return (long long)i * plan.stride; }

// The candidates [lo, hi] of lb after the pick p (0 .. m); lo == hi: lb is known.
ECDF_HD inline void ecdf_range(const EcdfPlan& plan, int B, int p, int& lo, int& hi) {
  if (p == 0) {
    lo = hi = 0;
    return;
  }
  const long long top = (long long)p * plan.stride;
  lo = (int)(top - plan.stride + 1);
  hi = top < B ? (int)top : B;
}

// N lower bounds over one ascending array: on return lo[k] = the first index of the entry range
// [lo[k], hi[k]) whose value is not below a[k] (hi[k] if there is none).  `steps` >= ecdf_steps of
// the largest entry range.
template <int N>
ECDF_HD inline void ecdf_lower_bound(const float* base, int (&lo)[N], int (&hi)[N], const float (&a)[N], int steps) {
  for (int it = 0; it < steps; ++it) {
    int mid[N];
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      mid[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
      v[k] = base[lo[k] < hi[k] ? mid[k] : 0];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool open = lo[k] < hi[k];
      const bool less = v[k] < a[k];
      lo[k] = open && less ? mid[k] + 1 : lo[k];
      hi[k] = open && !less ? mid[k] : hi[k];
    }
  }
}

// ge[k] = #{b : col[b] >= a[k]} for N queries against one column (col[0 .. B) ascending, spl its
// plan.m splitters); a NaN query gives -1.
template <int N>
ECDF_HD inline void ecdf_count_ge(const float* col, int B, const EcdfPlan& plan, const float* spl,
                                  const float (&a)[N], int (&ge)[N]) {
  int lo[N], hi[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    lo[k] = 0;
    hi[k] = plan.m;
  }
  ecdf_lower_bound<N>(spl, lo, hi, a, plan.pick_steps);
#pragma unroll
  for (int k = 0; k < N; ++k) ecdf_range(plan, B, lo[k], lo[k], hi[k]);
  ecdf_lower_bound<N>(col, lo, hi, a, plan.finish_steps);
#pragma unroll
  for (int k = 0; k < N; ++k) ge[k] = a[k] != a[k] ? -1 : B - lo[k];
}

}  // namespace expecto
