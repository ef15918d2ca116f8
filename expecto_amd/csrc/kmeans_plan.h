// Host half of the batched k-means (csrc/kmeans.hip): the limits, the per-problem tables' checks
// and the workspace layout.  Plain C++, no HIP: tests/kmeans_plan_driver.cpp builds it alone.
#pragma once

namespace expecto {

constexpr long long KM_MAX_N = 4096;      // 4 points per lane of a 1024-lane workgroup
constexpr long long KM_MAX_D = 128;
constexpr long long KM_MAX_K = 512;
constexpr long long KM_MAX_T = 8;
constexpr long long KM_MAX_P = 1LL << 20;
constexpr int KM_COLS = 8;                // int64 columns of a problem table row

// columns of a seeding row / of a Lloyd row (unused columns are ignored)
enum { KMS_K = 0, KMS_FIRST = 1, KMS_T = 2, KMS_U_OFF = 3, KMS_IDX_OFF = 4, KMS_C_OFF = 5 };
enum { KML_K = 0, KML_MAX_ITER = 1, KML_INIT_OFF = 2, KML_C_OFF = 3, KML_LABEL_OFF = 4 };

struct KmeansTotals {
  long long k_max = 0, t_max = 0;          // over the problems
  long long u_len = 0, idx_len = 0, c_len = 0, init_len = 0, label_len = 0;   // elements the offsets span
};

inline const char* kmeans_check_shape(long long n, long long d, long long ld, long long P) {
  if (P < 0 || P > KM_MAX_P) return "kmeans: problem count out of range (at most 1048576)";
  if (n < 1 || n > KM_MAX_N) return "kmeans: n must lie in [1, 4096]";
  if (d < 1 || d > KM_MAX_D) return "kmeans: d must lie in [1, 128]";
  if (ld < d) return "kmeans: row stride ld < d";
  return nullptr;
}

// An offset column: the first is 0 and block p + 1 starts at or after the end of block p.
inline bool kmeans_offsets_ok(const long long* prob, long long p, int col, long long len, long long* end) {
  const long long off = prob[p * KM_COLS + col];
  if (p == 0 ? off != 0 : off < *end) return false;
  *end = off + len;
  return true;
}

inline const char* kmeans_check_seeding(long long n, long long P, const long long* prob, KmeansTotals* tot) {
  *tot = KmeansTotals();
  for (long long p = 0; p < P; ++p) {
    const long long* r = prob + p * KM_COLS;
    const long long k = r[KMS_K], T = r[KMS_T];
    if (k < 1 || k > KM_MAX_K) return "kmeans_plusplus: k must lie in [1, 512]";
    if (k > n) return "kmeans_plusplus: k > n";
    if (T < 1 || T > KM_MAX_T) return "kmeans_plusplus: T must lie in [1, 8]";
    if (r[KMS_FIRST] < 0 || r[KMS_FIRST] >= n) return "kmeans_plusplus: first outside [0, n)";
    if (!kmeans_offsets_ok(prob, p, KMS_U_OFF, (k - 1) * T, &tot->u_len) ||
        !kmeans_offsets_ok(prob, p, KMS_IDX_OFF, k, &tot->idx_len) ||
        !kmeans_offsets_ok(prob, p, KMS_C_OFF, k, &tot->c_len))
      return "kmeans_plusplus: inconsistent offsets (first not 0, decreasing, or overlapping blocks)";
    if (k > tot->k_max) tot->k_max = k;
    if (T > tot->t_max) tot->t_max = T;
  }
  return nullptr;
}

inline const char* kmeans_check_lloyd(long long n, long long P, const long long* prob, KmeansTotals* tot) {
  *tot = KmeansTotals();
  for (long long p = 0; p < P; ++p) {
    const long long* r = prob + p * KM_COLS;
    const long long k = r[KML_K];
    if (k < 1 || k > KM_MAX_K) return "kmeans_lloyd: k must lie in [1, 512]";
    if (k > n) return "kmeans_lloyd: k > n";
    if (r[KML_MAX_ITER] < 1 || r[KML_MAX_ITER] > 0x7fffffffLL) return "kmeans_lloyd: max_iter must lie in [1, 2^31)";
    if (!kmeans_offsets_ok(prob, p, KML_INIT_OFF, k, &tot->init_len) ||
        !kmeans_offsets_ok(prob, p, KML_C_OFF, k, &tot->c_len) ||
        !kmeans_offsets_ok(prob, p, KML_LABEL_OFF, n, &tot->label_len))
      return "kmeans_lloyd: inconsistent offsets (first not 0, decreasing, or overlapping blocks)";
    if (k > tot->k_max) tot->k_max = k;
  }
  return nullptr;
}

// float64 elements of workspace per problem.  Seeding: closest-distance candidates dc[2][n, T] and their
// prefix sums cum[2][n, T], double-buffered.  Lloyd: new centres [k, d], dist [n], chain terms
// [max(k d, n)], member list int32 [n].
constexpr long long kmeans_seeding_stride(long long n, long long t_max) { return 4 * n * t_max; }
constexpr long long kmeans_lloyd_stride(long long n, long long d, long long k_max) {
  return k_max * d + n + (k_max * d > n ? k_max * d : n) + (n + 1) / 2;
}

inline long long kmeans_workspace_bytes(long long n, long long d, long long k_max, long long t_max, long long P) {
  if (kmeans_check_shape(n, d, d, P) || k_max < 1 || k_max > KM_MAX_K || t_max < 1 || t_max > KM_MAX_T) return 0;
  const long long a = kmeans_seeding_stride(n, t_max), b = kmeans_lloyd_stride(n, d, k_max);
  return 8 * P * (a > b ? a : b);
}

}  // namespace expecto
