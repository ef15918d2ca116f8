// Louvain clustering of one small point set (cluster_and_viz_louvain.py: Orange's Louvain(k) on the marks'
// SVD coordinates): the k-nearest-neighbour graph with Jaccard weights, one wave per point, and the
// community search, one wave per problem (a resolution and a visiting order) with the whole multi-level
// loop inside the kernel.  The arithmetic is the fixed one include/expecto_hip.h states: float64, products
// and sums rounded separately, every sum chained in the stated order, no floating-point atomics.  The
// search is sequential by definition (a node's move changes the next node's gains), so its parallelism
// is across problems; inside a problem the 64 lanes split a row, and what has to be a chain runs in lane 0.
#include <hip/hip_runtime.h>

#include <string>

#include "common.h"

#pragma clang fp contract(off)

namespace expecto {
namespace {

constexpr int LV_WAVE = 64;
constexpr int LV_MAX_N = 4096;
constexpr int LV_MAX_D = 128;
constexpr int LV_MAX_K = 64;
constexpr long long LV_MAX_NNZ = 1 << 20;
constexpr long long LV_MAX_P = 65535;
constexpr long long LV_MAX_PASSES = 1000;
constexpr long long LV_MAX_LEVELS = 64;
constexpr int LV_NONE = 0x7fffffff;
constexpr double LV_MIN_GAIN = 1e-7;

// ---- the graph -------------------------------------------------------------------------------

// nbr[i, 0..k): the k points of smallest (d2, index) to point i.  Lane l owns the candidates j = l, l + 64,
// ...; it takes them in ascending (d2, j), so its next candidate is its smallest above the last it gave.
__global__ __launch_bounds__(LV_WAVE) void knn_kernel(const double* __restrict__ X, int n, int d, long long ld, int k,
                                                      int* __restrict__ nbr) {
  __shared__ double D[LV_MAX_N];
  __shared__ double xi[LV_MAX_D];
  const int i = blockIdx.x, lane = threadIdx.x;
  for (int c = lane; c < d; c += LV_WAVE) xi[c] = X[(long long)i * ld + c];
  __syncthreads();
  for (int j = lane; j < n; j += LV_WAVE) {
    const double* x = X + (long long)j * ld;
    double s = 0.0;
    for (int c = 0; c < d; ++c) {
      const double t = xi[c] - x[c];
      s = s + t * t;
    }
    D[j] = s;
  }
  double lastv = -1.0;      // d2 >= 0: nothing given yet
  int lasti = -1;
  double bv = 0.0;
  int bj = LV_NONE;
  bool rescan = true;
  for (int t = 0; t < k; ++t) {
    if (rescan) {
      bv = __builtin_inf();
      bj = LV_NONE;
      for (int j = lane; j < n; j += LV_WAVE) {
        const double v = D[j];
        const bool after = v > lastv || (v == lastv && j > lasti);
        if (after && (v < bv || (v == bv && j < bj))) { bv = v; bj = j; }
      }
    }
    double wv = bv;
    int wj = bj;
    for (int m = LV_WAVE / 2; m > 0; m >>= 1) {
      const double ov = __shfl_xor(wv, m, LV_WAVE);
      const int oj = __shfl_xor(wj, m, LV_WAVE);
      if (oj != LV_NONE && (wj == LV_NONE || ov < wv || (ov == wv && oj < wj))) { wv = ov; wj = oj; }
    }
    wj = __shfl(wj, 0, LV_WAVE);
    if (lane == 0) nbr[(long long)i * k + t] = wj == LV_NONE ? i : wj;      // only a NaN distance leaves none
    rescan = wj != LV_NONE && wj == bj;
    if (rescan) { lastv = bv; lasti = bj; }
  }
}

// w[i, t] = |N(i) & N(j)| / (2k - |N(i) & N(j)|) for j = nbr[i, t], 0 for j = i.
__global__ __launch_bounds__(LV_WAVE) void jaccard_kernel(const int* __restrict__ nbr, int n, int k,
                                                          double* __restrict__ w) {
  __shared__ int Ni[LV_MAX_K];
  const int i = blockIdx.x, lane = threadIdx.x;
  if (lane < k) Ni[lane] = nbr[(long long)i * k + lane];
  __syncthreads();
  if (lane >= k) return;
  const int j = Ni[lane];
  double r = 0.0;
  if (j != i && j >= 0 && j < n) {
    int both = 0;
    for (int a = 0; a < k; ++a) {
      const int ja = nbr[(long long)j * k + a];
      for (int b = 0; b < k; ++b) both += Ni[b] == ja;
    }
    r = (double)both / (double)(2 * k - both);
  }
  w[(long long)i * k + lane] = r;
}

// ---- the communities -------------------------------------------------------------------------

struct Graph {
  const int* ptr;
  const int* idx;
  const double* w;
  int n;
};

struct LouvainShared {
  int comm[LV_MAX_N];          // node -> community slot
  double D[LV_MAX_N];          // a slot's total degree        (aggregation: the new row's accumulators)
  double kdeg[LV_MAX_N];       // a node's degree              (aggregation: stamps and member offsets)
  double L[LV_MAX_N];          // a slot's internal weight     (a long row's k_{v,c}; aggregation: renumbering)
};

__device__ __forceinline__ double bcast0(double v) { return __shfl(v, 0, LV_WAVE); }

// s = ((+0.0 + a[0]) + a[1]) + ... by lane 0, the value in every lane.
__device__ double chain_all(const double* a, int m) {
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < m; ++i) s = s + a[i];
  return bcast0(s);
}

// kdeg[v] = the row's sum in row order, a self-loop twice; returns 2m = the chain over v.
__device__ double degrees(LouvainShared& sh, const Graph& g) {
  for (int v = threadIdx.x; v < g.n; v += LV_WAVE) {
    double s = 0.0;
    for (int e = g.ptr[v]; e < g.ptr[v + 1]; ++e) {
      const double w = g.w[e];
      s = s + (g.idx[e] == v ? 2.0 * w : w);
    }
    sh.kdeg[v] = s;
  }
  __syncthreads();
  const double two_m = chain_all(sh.kdeg, g.n);
  __syncthreads();
  return two_m;
}

__device__ void singletons(LouvainShared& sh, int n) {
  for (int v = threadIdx.x; v < n; v += LV_WAVE) {
    sh.comm[v] = v;
    sh.D[v] = sh.kdeg[v];
  }
  __syncthreads();
}

// Q = the chain over slots c of L_c / m - gamma * (D_c / 2m)^2; L_c = the chain over the slot's nodes v
// ascending of lin_v, lin_v = the row-order sum of v's weights into its own slot towards x >= v.
__device__ double modularity(LouvainShared& sh, const Graph& g, double gamma, double two_m, double* tmp) {
  const int lane = threadIdx.x;
  for (int v = lane; v < g.n; v += LV_WAVE) {
    sh.L[v] = 0.0;
    const int cv = sh.comm[v];
    double s = 0.0;
    for (int e = g.ptr[v]; e < g.ptr[v + 1]; ++e) {
      const int x = g.idx[e];
      if (x >= v && sh.comm[x] == cv) s = s + g.w[e];
    }
    tmp[v] = s;
  }
  __threadfence_block();
  __syncthreads();
  if (lane == 0)
    for (int v = 0; v < g.n; ++v) {
      const int c = sh.comm[v];
      sh.L[c] = sh.L[c] + tmp[v];
    }
  __syncthreads();
  const double m = two_m * 0.5;
  for (int c = lane; c < g.n; c += LV_WAVE) {
    const double r = sh.D[c] / two_m;
    tmp[c] = sh.L[c] / m - gamma * (r * r);
  }
  __threadfence_block();
  __syncthreads();
  const double q = chain_all(tmp, g.n);
  __syncthreads();
  return q;
}

struct Cand {
  double g;
  int c;          // LV_NONE: no candidate
  int old;
};

__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {      // a before b
  if (a.c == LV_NONE) return false;
  if (b.c == LV_NONE) return true;
  return a.g > b.g || (a.g == b.g && (a.old > b.old || (a.old == b.old && a.c < b.c)));
}

// One pass of local moving; returns the number of nodes moved.
__device__ int move_pass(LouvainShared& sh, const Graph& g, const int* order, double gamma, double two_m) {
  const int lane = threadIdx.x;
  int moved = 0;
  for (int t = 0; t < g.n; ++t) {
    const int v = order ? order[t] : t;
    const int a = g.ptr[v], b = g.ptr[v + 1];
    __syncthreads();      // the previous visit's comm and D
    const int old = sh.comm[v];
    const double kv = sh.kdeg[v];
    if (lane == 0) sh.D[old] = sh.D[old] - kv;
    __syncthreads();
    Cand best = {0.0, LV_NONE, 0};
    if (b - a <= LV_WAVE) {
      // a row within the wave: lane l holds entry l; k_{v,c} by passing the row round in row order
      bool valid = lane < b - a;
      const int x = valid ? g.idx[a + lane] : v;
      const double w = valid ? g.w[a + lane] : 0.0;
      valid = valid && x != v;
      const int c = valid ? sh.comm[x] : -1;
      double s = 0.0;
      for (int u = 0; u < b - a; ++u) {
        const int cu = __shfl(c, u, LV_WAVE);
        const double wu = __shfl(w, u, LV_WAVE);
        if (cu == c) s = s + wu;
      }
      if (valid) best = {s - gamma * sh.D[c] * kv / two_m, c, c == old};
    } else {
      // a longer row: lane 0 chains k_{v,c} into L in row order
      for (int e = a + lane; e < b; e += LV_WAVE)
        if (g.idx[e] != v) sh.L[sh.comm[g.idx[e]]] = 0.0;
      __syncthreads();
      if (lane == 0)
        for (int e = a; e < b; ++e) {
          const int x = g.idx[e];
          if (x != v) sh.L[sh.comm[x]] = sh.L[sh.comm[x]] + g.w[e];
        }
      __syncthreads();
      for (int e = a + lane; e < b; e += LV_WAVE) {
        const int x = g.idx[e];
        if (x == v) continue;
        const int c = sh.comm[x];
        const Cand cand = {sh.L[c] - gamma * sh.D[c] * kv / two_m, c, c == old};
        if (better(cand, best)) best = cand;
      }
    }
    const bool has_old = __any(best.c != LV_NONE && best.old);
    for (int m = LV_WAVE / 2; m > 0; m >>= 1) {
      const Cand o = {__shfl_xor(best.g, m, LV_WAVE), __shfl_xor(best.c, m, LV_WAVE), __shfl_xor(best.old, m, LV_WAVE)};
      if (better(o, best)) best = o;
    }
    int to = __shfl(best.c, 0, LV_WAVE);
    const double tg = bcast0(best.g);
    if (to == LV_NONE) {
      to = old;
    } else if (!has_old) {
      const double stay = 0.0 - gamma * sh.D[old] * kv / two_m;
      if (!(tg > stay)) to = old;
    }
    if (lane == 0) {
      sh.D[to] = sh.D[to] + kv;
      sh.comm[v] = to;
    }
    moved += to != old;
  }
  __syncthreads();
  return moved;
}

struct Buffers {
  int* ptr;
  int* idx;
  double* w;
};

// The graph of the communities: slots renumbered by smallest member, labels carried along, rows in
// ascending neighbour id, internal weight (each edge once, from its lower end) as a self-loop.
__device__ Graph aggregate(LouvainShared& sh, const Graph& g, int* lab, int n0, int* members, const Buffers& out,
                           int cap) {
  const int lane = threadIdx.x;
  int* minm = reinterpret_cast<int*>(sh.L);
  int* newid = minm + LV_MAX_N;
  double* acc = sh.D;
  int* stamp = reinterpret_cast<int*>(sh.kdeg);
  int* off = stamp + LV_MAX_N;
  const unsigned long long below = (1ULL << lane) - 1ULL;

  for (int c = lane; c < g.n; c += LV_WAVE) minm[c] = LV_NONE;
  __syncthreads();
  for (int v = lane; v < g.n; v += LV_WAVE) atomicMin(&minm[sh.comm[v]], v);
  __syncthreads();
  int n_new = 0;
  for (int v0 = 0; v0 < g.n; v0 += LV_WAVE) {
    const int v = v0 + lane;
    const bool first = v < g.n && minm[sh.comm[v]] == v;
    const unsigned long long mask = __ballot(first);
    if (first) newid[sh.comm[v]] = n_new + __popcll(mask & below);
    n_new += __popcll(mask);
  }
  __syncthreads();
  for (int i = lane; i < n0; i += LV_WAVE) lab[i] = newid[sh.comm[lab[i]]];
  __syncthreads();
  for (int v = lane; v < g.n; v += LV_WAVE) sh.comm[v] = newid[sh.comm[v]];
  for (int c = lane; c < n_new; c += LV_WAVE) {
    off[c] = 0;
    stamp[c] = -1;
  }
  __syncthreads();
  for (int v = lane; v < g.n; v += LV_WAVE) atomicAdd(&off[sh.comm[v]], 1);
  __syncthreads();
  if (lane == 0) {
    int run = 0;
    for (int c = 0; c < n_new; ++c) {
      const int m = off[c];
      off[c] = run;
      run += m;
    }
    for (int v = 0; v < g.n; ++v) members[off[sh.comm[v]]++] = v;      // off[c] ends as the end of c's members
  }
  __threadfence_block();
  __syncthreads();

  int filled = 0;
  for (int c = 0; c < n_new; ++c) {
    if (lane == 0) {
      double loop = 0.0;
      bool has_loop = false;
      for (int m = c ? off[c - 1] : 0; m < off[c]; ++m) {
        const int u = members[m];
        for (int e = g.ptr[u]; e < g.ptr[u + 1]; ++e) {
          const int x = g.idx[e];
          const int cx = sh.comm[x];
          const double w = g.w[e];
          if (cx == c) {
            if (x >= u) {
              loop = loop + w;
              has_loop = true;
            }
          } else {
            if (stamp[cx] != c) {
              stamp[cx] = c;
              acc[cx] = 0.0;
            }
            acc[cx] = acc[cx] + w;
          }
        }
      }
      if (has_loop) {
        stamp[c] = c;
        acc[c] = loop;
      }
      out.ptr[c] = filled;
    }
    __syncthreads();
    for (int x0 = 0; x0 < n_new; x0 += LV_WAVE) {
      const int x = x0 + lane;
      const bool in = x < n_new && stamp[x] == c;
      const unsigned long long mask = __ballot(in);
      const int pos = filled + __popcll(mask & below);
      if (in && pos < cap) {
        out.idx[pos] = x;
        out.w[pos] = acc[x];
      }
      filled += __popcll(mask);
    }
    __syncthreads();
  }
  if (lane == 0) out.ptr[n_new] = filled;
  __threadfence_block();
  __syncthreads();
  return Graph{out.ptr, out.idx, out.w, n_new};
}

__global__ __launch_bounds__(LV_WAVE) void louvain_kernel(
    const int* __restrict__ indptr, const int* __restrict__ indices, const double* __restrict__ weights, int n, int nnz,
    const double* __restrict__ gammas, const int* __restrict__ perm, int max_passes, int max_levels,
    int* __restrict__ labels, double* __restrict__ modularity_out, int* __restrict__ counters, double* __restrict__ ws,
    long long stride, int cap) {
  __shared__ LouvainShared sh;
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  int* lab = labels + (long long)p * n;
  const int* order = perm + (long long)p * n;
  const double gamma = gammas[p];

  // the graph and the order are device memory the host never saw: a problem whose copy would index
  // outside them is passed over
  int bad = 0;
  for (int v = lane; v < n; v += LV_WAVE) {
    const int a = indptr[v], b = indptr[v + 1];
    if (a < 0 || b < a || b > nnz || order[v] < 0 || order[v] >= n) bad = 1;
  }
  if (lane == 0 && (indptr[0] != 0 || indptr[n] != nnz)) bad = 1;
  for (int e = lane; e < nnz; e += LV_WAVE)
    if (indices[e] < 0 || indices[e] >= n) bad = 1;
  if (__syncthreads_or(bad)) {
    if (lane == 0) {
      modularity_out[p] = 0.0;
      counters[4 * p + 0] = 0;
      counters[4 * p + 1] = 0;
      counters[4 * p + 2] = 0;
      counters[4 * p + 3] = EXPECTO_LOUVAIN_BAD_GRAPH;
    }
    return;
  }

  double* base = ws + (long long)p * stride;
  double* tmp = base + 2LL * cap;
  int* ints = reinterpret_cast<int*>(tmp + n);
  const Buffers buf[2] = {{ints + 2LL * cap, ints, base}, {ints + 2LL * cap + (n + 1), ints + cap, base + cap}};
  int* members = ints + 2LL * cap + 2LL * (n + 1);

  Graph g = {indptr, indices, weights, n};
  for (int v = lane; v < n; v += LV_WAVE) lab[v] = v;
  double two_m = degrees(sh, g);
  int n_levels = 0, n_passes = 0, flags = 0;
  double Q = 0.0;
  if (two_m != 0.0) {
    singletons(sh, n);
    Q = modularity(sh, g, gamma, two_m, tmp);
    bool done = false;
    for (int level = 0; level < max_levels; ++level) {
      const double q_start = Q;
      int moved = 0;
      bool stop = false;
      for (int pass = 0; pass < max_passes; ++pass) {
        const int mv = move_pass(sh, g, level == 0 ? order : nullptr, gamma, two_m);
        n_passes += 1;
        moved += mv;
        const double q = modularity(sh, g, gamma, two_m, tmp);
        const double rise = q - Q;
        Q = q;
        if (mv == 0 || rise < LV_MIN_GAIN) {
          stop = true;
          break;
        }
      }
      if (!stop) flags |= EXPECTO_LOUVAIN_PASS_BOUND;
      if (moved == 0) {
        done = true;
        break;
      }
      g = aggregate(sh, g, lab, n, members, buf[level & 1], cap);
      n_levels += 1;
      two_m = degrees(sh, g);
      singletons(sh, g.n);
      if (Q - q_start < LV_MIN_GAIN) {
        done = true;
        break;
      }
    }
    if (!done) flags |= EXPECTO_LOUVAIN_LEVEL_BOUND;
  }
  if (lane == 0) {
    modularity_out[p] = Q;
    counters[4 * p + 0] = g.n;
    counters[4 * p + 1] = n_levels;
    counters[4 * p + 2] = n_passes;
    counters[4 * p + 3] = flags;
  }
}

inline long long louvain_cap(long long n, long long nnz) { return nnz + n; }

// float64 elements of one problem's workspace: two graphs' weights, a column of n, then as int32 two
// graphs' indices and row pointers and the member list
inline long long louvain_stride(long long n, long long nnz) {
  const long long cap = louvain_cap(n, nnz);
  const long long ints = 2 * cap + 2 * (n + 1) + n;
  return 2 * cap + n + (ints + 1) / 2;
}

inline const char* louvain_check_shape(long long n, long long nnz, long long P) {
  if (n < 1 || n > LV_MAX_N) return "louvain: n must lie in [1, 4096]";
  if (nnz < 0 || nnz > LV_MAX_NNZ) return "louvain: nnz must lie in [0, 1048576]";
  if (P < 0 || P > LV_MAX_P) return "louvain: problem count must lie in [0, 65535]";
  return nullptr;
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_knn_jaccard(const double* X, long long n, long long d, long long ld, long long k, int* nbr, double* w,
                        void* stream) {
  EXPECTO_REQUIRE(n >= 1 && n <= LV_MAX_N, "knn_jaccard: n must lie in [1, 4096]");
  EXPECTO_REQUIRE(d >= 1 && d <= LV_MAX_D, "knn_jaccard: d must lie in [1, 128]");
  EXPECTO_REQUIRE(k >= 1 && k <= LV_MAX_K, "knn_jaccard: k must lie in [1, 64]");
  EXPECTO_REQUIRE(k <= n, "knn_jaccard: k > n");
  EXPECTO_REQUIRE(ld >= d, "knn_jaccard: ld < d");
  EXPECTO_REQUIRE(X && nbr && w, "null argument");
  knn_kernel<<<dim3((unsigned)n), dim3(LV_WAVE), 0, as_stream(stream)>>>(X, (int)n, (int)d, ld, (int)k, nbr);
  if (int st = check_launch("knn_jaccard")) return st;
  jaccard_kernel<<<dim3((unsigned)n), dim3(LV_WAVE), 0, as_stream(stream)>>>(nbr, (int)n, (int)k, w);
  return check_launch("knn_jaccard");
}

size_t expecto_louvain_workspace(long long n, long long nnz, long long P) {
  if (louvain_check_shape(n, nnz, P)) return 0;
  return (size_t)(8 * P * louvain_stride(n, nnz));
}

int expecto_louvain(const int* indptr, const int* indices, const double* weights, long long n, long long nnz,
                    long long P, const double* gamma, const int* perm, long long max_passes, long long max_levels,
                    int* labels, double* modularity, int* counters, void* workspace, size_t workspace_bytes,
                    void* stream) {
  if (const char* err = louvain_check_shape(n, nnz, P)) EXPECTO_REQUIRE(false, err);
  EXPECTO_REQUIRE(max_passes >= 1 && max_passes <= LV_MAX_PASSES, "louvain: max_passes must lie in [1, 1000]");
  EXPECTO_REQUIRE(max_levels >= 1 && max_levels <= LV_MAX_LEVELS, "louvain: max_levels must lie in [1, 64]");
  if (P == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(indptr && (nnz == 0 || (indices && weights)) && gamma && perm && labels && modularity && counters &&
                      workspace,
                  "null argument");
  EXPECTO_REQUIRE((unsigned long long)workspace_bytes >= 8ULL * P * louvain_stride(n, nnz),
                  "louvain: workspace too small (expecto_louvain_workspace)");
  EXPECTO_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "louvain: workspace not 8-byte aligned");
  louvain_kernel<<<dim3((unsigned)P), dim3(LV_WAVE), 0, as_stream(stream)>>>(
      indptr, indices, weights, (int)n, (int)nnz, gamma, perm, (int)max_passes, (int)max_levels, labels, modularity,
      counters, static_cast<double*>(workspace), louvain_stride(n, nnz), (int)louvain_cap(n, nnz));
  return check_launch("louvain");
}

}  // extern "C"
