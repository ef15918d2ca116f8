// Batched k-means of one small matrix (cluster_and_viz.py:45-58 and its commented-out elbow sweep):
// sklearn's greedy k-means++ seeding and its Lloyd iteration, one workgroup per problem, the whole
// step / iteration loop inside the kernel.  The arithmetic is the fixed one include/expecto_hip.h
// states: float64, products and sums rounded separately, every sum that the contract calls sequential
// chained in one lane in ascending order (the terms are computed by all lanes first), no atomics.
// A problem's bits depend on nothing but its own inputs.  The tables' checks and the workspace layout
// are host code (kmeans_plan.h).
#include <hip/hip_runtime.h>

#include <string>

#include "common.h"
#include "kmeans_plan.h"

#pragma clang fp contract(off)

namespace expecto {
namespace {

constexpr int KM_THREADS = 1024;
constexpr int KM_PTS = 4;                  // points per lane: KM_MAX_N / KM_THREADS
constexpr int KM_GROUP = 8;                // centres (Lloyd) or candidates (seeding) per pass over a point's row
constexpr int KM_CHUNK = 2048;             // doubles of centres staged in LDS per E-step chunk (>= KM_GROUP * KM_MAX_D)
constexpr int KM_CHAIN = 8;                // loads in flight ahead of a chain's adds
static_assert(KM_PTS * KM_THREADS == KM_MAX_N && KM_GROUP == KM_MAX_T && KM_CHUNK >= KM_GROUP * KM_MAX_D, "limits");

// s = ((+0.0 + a[0]) + a[stride]) + ...: one lane, m terms, the loads issued KM_CHAIN ahead of the adds.
// With `prefix` every partial sum is stored too (np.cumsum).
__device__ __forceinline__ double chain_sum(const double* a, long long stride, int m, double* prefix) {
  double s = 0.0;
  int i = 0;
  for (; i + KM_CHAIN <= m; i += KM_CHAIN) {
    double t[KM_CHAIN];
#pragma unroll
    for (int u = 0; u < KM_CHAIN; ++u) t[u] = a[(long long)(i + u) * stride];
#pragma unroll
    for (int u = 0; u < KM_CHAIN; ++u) {
      s = s + t[u];
      if (prefix) prefix[(long long)(i + u) * stride] = s;
    }
  }
  for (; i < m; ++i) {
    s = s + a[(long long)i * stride];
    if (prefix) prefix[(long long)i * stride] = s;
  }
  return s;
}

// ---- seeding ---------------------------------------------------------------------------------
//
// Step c has Tc candidates (one, `first`, at c = 0).  All lanes: dc[i, t] = min(closest[i],
// d2(X[i], X[cand[t]])), a point's row read once for all candidates.  Lanes t < Tc of wave 0: the
// prefix sums cum[., t] of dc[., t], each a chain; cum[n-1, t] is the candidate's potential.  The
// winner's dc and cum columns are the next step's closest and cum, so nothing is recomputed.  dc and
// cum are [n, T] (a step's T chains read one line per point) and double-buffered in the workspace.
__global__ __launch_bounds__(KM_THREADS) void kmeans_plusplus_kernel(
    const double* __restrict__ X, int n, int d, long long ld, const long long* __restrict__ prob,
    const double* __restrict__ u, long long u_len, int* __restrict__ idx_out, long long idx_len,
    double* __restrict__ centres, long long c_len, double* __restrict__ ws, long long ws_stride) {
  __shared__ double crow[KM_GROUP][KM_MAX_D];
  __shared__ double val[KM_GROUP];
  __shared__ int cand[KM_GROUP];
  __shared__ int win_s;
  __shared__ double pot_s;

  const int tid = threadIdx.x;
  const long long* row = prob + (long long)blockIdx.x * KM_COLS;
  const long long k = row[KMS_K], first = row[KMS_FIRST], T = row[KMS_T];
  const long long u_off = row[KMS_U_OFF], i_off = row[KMS_IDX_OFF], c_off = row[KMS_C_OFF];
  // the device copy of the table is not the one the host checked: a row that does not fit is passed over
  if (k < 1 || k > n || k > KM_MAX_K || T < 1 || T > KM_MAX_T || first < 0 || first >= n || u_off < 0 ||
      u_off + (k - 1) * T > u_len || i_off < 0 || i_off + k > idx_len || c_off < 0 || c_off + k > c_len ||
      4LL * n * T > ws_stride)
    return;
  const double* up = u + u_off;
  int* idx = idx_out + i_off;
  double* cen = centres + c_off * d;
  double* base = ws + (long long)blockIdx.x * ws_stride;
  const long long nT = (long long)n * T;
  int cur = 0;        // buffer this step writes
  int win = 0;        // previous step's winner

  for (int c = 0; c < (int)k; ++c) {
    const int Tc = c == 0 ? 1 : (int)T;
    double* dc = base + cur * nT;
    double* cum = base + (2 + cur) * nT;
    const double* closest = base + (cur ^ 1) * nT + win;
    const double* pcum = base + (2 + (cur ^ 1)) * nT + win;

    // candidates: np.searchsorted(cum, u * pot, 'left') clipped to n - 1.  cum never decreases, so at most
    // one i has cum[i-1] < v <= cum[i]: a single writer per candidate.
    if (c == 0) {
      if (tid == 0) cand[0] = (int)first;
    } else if (tid < Tc) {
      val[tid] = up[(long long)(c - 1) * T + tid] * pot_s;
      cand[tid] = n - 1;
    }
    __syncthreads();
    if (c > 0) {
      for (int i = tid; i < n; i += KM_THREADS) {
        const double hi = pcum[(long long)i * T];
        const bool has_lo = i > 0;
        const double lo = has_lo ? pcum[(long long)(i - 1) * T] : 0.0;
        for (int t = 0; t < Tc; ++t) {
          const double v = val[t];
          if (hi >= v && (!has_lo || lo < v)) cand[t] = i;
        }
      }
      __syncthreads();
    }
    for (int e = tid; e < Tc * d; e += KM_THREADS) crow[e / d][e % d] = X[(long long)cand[e / d] * ld + e % d];
    __syncthreads();

    for (int i = tid; i < n; i += KM_THREADS) {
      const double* x = X + (long long)i * ld;
      double s[KM_GROUP];
#pragma unroll
      for (int t = 0; t < KM_GROUP; ++t) s[t] = 0.0;
      for (int j = 0; j < d; ++j) {
        const double xv = x[j];
#pragma unroll
        for (int t = 0; t < KM_GROUP; ++t) {
          if (t < Tc) {
            const double q = xv - crow[t][j];
            s[t] = s[t] + q * q;
          }
        }
      }
      const double cl = c == 0 ? __builtin_inf() : closest[(long long)i * T];
#pragma unroll
      for (int t = 0; t < KM_GROUP; ++t)
        if (t < Tc) dc[(long long)i * T + t] = s[t] < cl ? s[t] : cl;
    }
    __syncthreads();

    if (tid < Tc) chain_sum(dc + tid, T, n, cum + tid);
    __syncthreads();

    if (tid == 0) {
      int w = 0;
      double best = cum[(long long)(n - 1) * T];
      for (int t = 1; t < Tc; ++t) {
        const double pt = cum[(long long)(n - 1) * T + t];
        if (pt < best) { best = pt; w = t; }
      }
      win_s = w;
      pot_s = best;
      idx[c] = cand[w];
    }
    __syncthreads();
    win = win_s;
    for (int j = tid; j < d; j += KM_THREADS) cen[(long long)c * d + j] = crow[win][j];
    cur ^= 1;
    __syncthreads();      // cand, val and crow are rewritten by the next step
  }
}

// ---- Lloyd -----------------------------------------------------------------------------------

struct LloydShared {
  double cl[KM_CHUNK];           // a chunk of centres (E-step)
  double rv[KM_THREADS];         // argmax reduction (relocation)
  int ri[KM_THREADS];
  int mlab[KM_MAX_N];            // the M-step's labels: `label` after relocation
  int cnt[KM_MAX_K];
  int off[KM_MAX_K + 1];
  int empty[KM_MAX_K];
  int n_empty;
  double shift;
};

// label[i] = the lowest c of minimal d2(X[i], C[c]), dist[i] that minimum.  The centres pass through
// LDS in chunks; a lane holds KM_GROUP running sums per point, so a point's row is read once per
// KM_GROUP centres.  Returns whether any label differs from the one stored before (all lanes agree).
__device__ int e_step(LloydShared& sh, const double* __restrict__ X, int n, int d, long long ld, int k,
                      const double* C, int* label, double* dist, bool first_iter) {
  const int tid = threadIdx.x;
  double best[KM_PTS];
  int bc[KM_PTS];
#pragma unroll
  for (int q = 0; q < KM_PTS; ++q) { best[q] = __builtin_inf(); bc[q] = 0; }
  const int per_chunk = KM_CHUNK / d;
  for (int c0 = 0; c0 < k; c0 += per_chunk) {
    const int nc = k - c0 < per_chunk ? k - c0 : per_chunk;
    __syncthreads();
    for (int e = tid; e < nc * d; e += KM_THREADS) sh.cl[e] = C[(long long)c0 * d + e];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KM_PTS; ++q) {
      const int i = tid + q * KM_THREADS;
      if (i >= n) continue;
      const double* x = X + (long long)i * ld;
      for (int g = 0; g < nc; g += KM_GROUP) {
        const int ng = nc - g < KM_GROUP ? nc - g : KM_GROUP;
        const double* cg = sh.cl + g * d;
        double s[KM_GROUP];
#pragma unroll
        for (int v = 0; v < KM_GROUP; ++v) s[v] = 0.0;
        if (ng == KM_GROUP) {
          for (int j = 0; j < d; ++j) {
            const double xv = x[j];
#pragma unroll
            for (int v = 0; v < KM_GROUP; ++v) {
              const double t = xv - cg[v * d + j];
              s[v] = s[v] + t * t;
            }
          }
        } else {
          for (int j = 0; j < d; ++j) {
            const double xv = x[j];
#pragma unroll
            for (int v = 0; v < KM_GROUP; ++v) {
              if (v < ng) {
                const double t = xv - cg[v * d + j];
                s[v] = s[v] + t * t;
              }
            }
          }
        }
#pragma unroll
        for (int v = 0; v < KM_GROUP; ++v)
          if (v < ng && s[v] < best[q]) { best[q] = s[v]; bc[q] = c0 + g + v; }
      }
    }
  }
  int changed = first_iter ? 1 : 0;
#pragma unroll
  for (int q = 0; q < KM_PTS; ++q) {
    const int i = tid + q * KM_THREADS;
    if (i >= n) continue;
    if (label[i] != bc[q]) changed = 1;
    label[i] = bc[q];
    dist[i] = best[q];
  }
  return __syncthreads_or(changed);
}

// The point of largest dist (>= 0; a taken point holds -1), the lower index on ties: exact, so a tree.
__device__ int argmax_point(LloydShared& sh, const double* dist, int n) {
  const int tid = threadIdx.x;
  double bv = -2.0;
  int bi = 0x7fffffff;
  for (int i = tid; i < n; i += KM_THREADS) {
    const double v = dist[i];
    if (v > bv) { bv = v; bi = i; }      // ascending i: the lower index stays on ties
  }
  sh.rv[tid] = bv;
  sh.ri[tid] = bi;
  __syncthreads();
  for (int h = KM_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const double ov = sh.rv[tid + h];
      const int oi = sh.ri[tid + h];
      if (ov > sh.rv[tid] || (ov == sh.rv[tid] && oi < sh.ri[tid])) { sh.rv[tid] = ov; sh.ri[tid] = oi; }
    }
    __syncthreads();
  }
  const int r = sh.ri[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_lloyd_kernel(
    const double* __restrict__ X, int n, int d, long long ld, const long long* __restrict__ prob,
    const double* __restrict__ tol, const double* __restrict__ init, long long init_len, int* __restrict__ labels,
    long long label_len, double* __restrict__ centres, long long c_len, double* __restrict__ inertia,
    int* __restrict__ n_iter, double* __restrict__ ws, long long ws_stride) {
  __shared__ LloydShared sh;
  const int tid = threadIdx.x;
  const long long* row = prob + (long long)blockIdx.x * KM_COLS;
  const long long kk = row[KML_K], max_iter = row[KML_MAX_ITER];
  const long long in_off = row[KML_INIT_OFF], c_off = row[KML_C_OFF], l_off = row[KML_LABEL_OFF];
  const long long kd = kk * d;
  if (kk < 1 || kk > n || kk > KM_MAX_K || max_iter < 1 || in_off < 0 || in_off + kk > init_len || c_off < 0 ||
      c_off + kk > c_len || l_off < 0 || l_off + n > label_len || kmeans_lloyd_stride(n, d, kk) > ws_stride)
    return;
  const int k = (int)kk;
  double* C = centres + c_off * d;
  int* label = labels + l_off;
  double* Cn = ws + (long long)blockIdx.x * ws_stride;
  double* dist = Cn + kd;
  double* terms = dist + n;
  int* members = reinterpret_cast<int*>(terms + (kd > n ? kd : n));
  const double tolp = tol[blockIdx.x];

  for (long long e = tid; e < kd; e += KM_THREADS) C[e] = init[in_off * d + e];
  __syncthreads();

  bool strict = false;
  int iters = 0;
  for (long long it = 0; it < max_iter; ++it) {
    const int changed = e_step(sh, X, n, d, ld, k, C, label, dist, it == 0);

    // member counts, one lane per cluster over the labels in LDS
    for (int i = tid; i < n; i += KM_THREADS) sh.mlab[i] = label[i];
    __syncthreads();
    if (tid < k) {
      int m = 0;
      for (int i = 0; i < n; ++i) m += sh.mlab[i] == tid;
      sh.cnt[tid] = m;
    }
    __syncthreads();
    if (tid == 0) {
      int e = 0;
      for (int c = 0; c < k; ++c)
        if (sh.cnt[c] == 0) sh.empty[e++] = c;
      sh.n_empty = e;
    }
    __syncthreads();
    // relocation: the r-th empty cluster (ascending) takes the point of r-th largest dist
    const int n_empty = sh.n_empty;
    for (int r = 0; r < n_empty; ++r) {
      const int far = argmax_point(sh, dist, n);
      if (tid == 0) {
        sh.cnt[sh.mlab[far]] -= 1;
        sh.mlab[far] = sh.empty[r];
        sh.cnt[sh.empty[r]] = 1;
        dist[far] = -1.0;
      }
      __syncthreads();
    }
    // member lists: ascending points per cluster (a stable compaction)
    if (tid == 0) {
      int o = 0;
      for (int c = 0; c < k; ++c) { sh.off[c] = o; o += sh.cnt[c]; }
      sh.off[k] = o;
    }
    __syncthreads();
    if (tid < k) {
      int o = sh.off[tid];
      for (int i = 0; i < n; ++i)
        if (sh.mlab[i] == tid) members[o++] = i;
    }
    __syncthreads();

    // M-step: one lane per (c, j), a chain over the members; then the shift's terms
    for (int e = tid; e < (int)kd; e += KM_THREADS) {
      const int c = e / d, j = e % d;
      const int m0 = sh.off[c], m1 = sh.off[c + 1];
      double v = C[e];
      if (m1 > m0) {
        double s = 0.0;
        int m = m0;
        for (; m + KM_CHAIN <= m1; m += KM_CHAIN) {
          double t[KM_CHAIN];
#pragma unroll
          for (int w = 0; w < KM_CHAIN; ++w) t[w] = X[(long long)members[m + w] * ld + j];
#pragma unroll
          for (int w = 0; w < KM_CHAIN; ++w) s = s + t[w];
        }
        for (; m < m1; ++m) s = s + X[(long long)members[m] * ld + j];
        v = s / (double)(m1 - m0);
      }
      Cn[e] = v;
      const double t = v - C[e];
      terms[e] = t * t;
    }
    __syncthreads();
    if (tid == 0) sh.shift = chain_sum(terms, 1, (int)kd, nullptr);
    for (int e = tid; e < (int)kd; e += KM_THREADS) C[e] = Cn[e];
    __syncthreads();
    iters = (int)(it + 1);
    if (!changed) { strict = true; break; }
    if (sh.shift <= tolp) break;
  }

  if (!strict) e_step(sh, X, n, d, ld, k, C, label, dist, false);
  __syncthreads();
  for (int i = tid; i < n; i += KM_THREADS) {
    const double* x = X + (long long)i * ld;
    const double* c = C + (long long)label[i] * d;
    double s = 0.0;
    for (int j = 0; j < d; ++j) {
      const double t = x[j] - c[j];
      s = s + t * t;
    }
    terms[i] = s;
  }
  __syncthreads();
  if (tid == 0) {
    inertia[blockIdx.x] = chain_sum(terms, 1, n, nullptr);
    n_iter[blockIdx.x] = iters;
  }
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

size_t expecto_kmeans_workspace(long long n, long long d, long long k_max, long long t_max, long long P) {
  return (size_t)kmeans_workspace_bytes(n, d, k_max, t_max, P);
}

int expecto_kmeans_plusplus(const double* X, long long n, long long d, long long ld, long long P,
                            const long long* prob_host, const long long* prob, const double* u, int* idx,
                            double* centres, void* workspace, size_t workspace_bytes, void* stream) {
  if (const char* err = kmeans_check_shape(n, d, ld, P)) EXPECTO_REQUIRE(false, err);
  if (P == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(prob_host, "null argument");
  KmeansTotals tot;
  if (const char* err = kmeans_check_seeding(n, P, prob_host, &tot)) EXPECTO_REQUIRE(false, err);
  EXPECTO_REQUIRE(X && prob && idx && centres && workspace && (u || tot.u_len == 0), "null argument");
  const long long stride = kmeans_seeding_stride(n, tot.t_max);
  EXPECTO_REQUIRE((unsigned long long)workspace_bytes >= 8ULL * P * stride,
                  "kmeans_plusplus: workspace too small (expecto_kmeans_workspace)");
  EXPECTO_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "kmeans_plusplus: workspace not 8-byte aligned");
  kmeans_plusplus_kernel<<<dim3((unsigned)P), dim3(KM_THREADS), 0, as_stream(stream)>>>(
      X, (int)n, (int)d, ld, prob, u, tot.u_len, idx, tot.idx_len, centres, tot.c_len, static_cast<double*>(workspace),
      stride);
  return check_launch("kmeans_plusplus");
}

int expecto_kmeans_lloyd(const double* X, long long n, long long d, long long ld, long long P,
                         const long long* prob_host, const long long* prob, const double* tol, const double* init,
                         int* labels, double* centres, double* inertia, int* n_iter, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (const char* err = kmeans_check_shape(n, d, ld, P)) EXPECTO_REQUIRE(false, err);
  if (P == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(prob_host, "null argument");
  KmeansTotals tot;
  if (const char* err = kmeans_check_lloyd(n, P, prob_host, &tot)) EXPECTO_REQUIRE(false, err);
  EXPECTO_REQUIRE(X && prob && tol && init && labels && centres && inertia && n_iter && workspace, "null argument");
  const long long stride = kmeans_lloyd_stride(n, d, tot.k_max);
  EXPECTO_REQUIRE((unsigned long long)workspace_bytes >= 8ULL * P * stride,
                  "kmeans_lloyd: workspace too small (expecto_kmeans_workspace)");
  EXPECTO_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "kmeans_lloyd: workspace not 8-byte aligned");
  kmeans_lloyd_kernel<<<dim3((unsigned)P), dim3(KM_THREADS), 0, as_stream(stream)>>>(
      X, (int)n, (int)d, ld, prob, tol, init, tot.init_len, labels, tot.label_len, centres, tot.c_len, inertia, n_iter,
      static_cast<double*>(workspace), stride);
  return check_launch("kmeans_lloyd");
}

}  // extern "C"
