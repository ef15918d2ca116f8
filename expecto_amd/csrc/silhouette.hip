// Silhouette of the cuts of a Ward tree (interpret_features_grouped.py:120-144, the sweep the
// reference has commented out): per-point distance sums of tree nodes, then the silhouette samples
// of every cut, from the exact distances of expecto_pairwise_euclidean.  The planner that lists the
// nodes and the cuts is host Python (expecto_amd/interpret_features.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "common.h"

namespace expecto {
namespace {

constexpr int SIL_THREADS = 256;
constexpr int SIL_UNROLL = 8;               // member rows in flight per lane in the node sums
constexpr int SQ_TILE = 32;
constexpr long long SIL_MAX_N = 1LL << 20;  // grid.y = ceil(n / 32) of the square expansion stays below 65536

// condensed [n(n-1)/2] -> square [n, n], both triangles and a +0.0 diagonal.  A workgroup takes one
// 32 x 32 tile (bi <= bj) of the upper triangle: row-contiguous reads of the condensed rows, the tile
// stored as it is and, through LDS, transposed, so both stores are row-contiguous too.
__global__ __launch_bounds__(SIL_THREADS) void square_distances_kernel(const double* __restrict__ cond, long long n,
                                                                       double* __restrict__ sq) {
  __shared__ double tile[SQ_TILE][SQ_TILE + 1];
  if (blockIdx.y > blockIdx.x) return;   // whole workgroup: tiles below the diagonal are the transposes
  const long long i0 = (long long)blockIdx.y * SQ_TILE, j0 = (long long)blockIdx.x * SQ_TILE;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int li = ty + 8 * r;
    const long long i = i0 + li, j = j0 + tx;
    double v = 0.0;
    if (i < n && j < n) {
      if (i != j) {
        const long long lo = i < j ? i : j, hi = i < j ? j : i;
        v = cond[n * lo - lo * (lo + 1) / 2 + (hi - lo - 1)];
      }
      sq[i * n + j] = v;
    }
    tile[li][tx] = v;
  }
  __syncthreads();
  if (blockIdx.y == blockIdx.x) return;  // a diagonal tile is its own transpose
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lj = ty + 8 * r;
    const long long j = j0 + lj, i = i0 + tx;
    if (i < n && j < n) sq[j * n + i] = tile[tx][lj];
  }
}

// d(i, j) of either layout.  A member outside [0, n) is not a point: it reads nothing and adds +0.0.
template <bool SQUARE>
__device__ __forceinline__ double dist_of(const double* __restrict__ D, long long n, long long i, long long j) {
  if (j < 0 || j >= n) return 0.0;
  if (SQUARE) return D[j * n + i];
  if (i == j) return 0.0;
  const long long lo = i < j ? i : j, hi = i < j ? j : i;
  return D[n * lo - lo * (lo + 1) / 2 + (hi - lo - 1)];
}

// S[v, i] = ((+0.0 + d(i, j1)) + d(i, j2)) + ... over the members j1 < j2 < ... of node v as the CSR
// lists them: one lane per (node, point), consecutive lanes consecutive points, a single chain of
// rounded adds per lane.  The member index is uniform over the workgroup; SIL_UNROLL loads are issued
// before their adds.  Offsets are clamped to [0, n_members], so the trip count follows from the
// arguments and no list entry past the array is read.
template <bool SQUARE>
__global__ __launch_bounds__(SIL_THREADS) void node_sums_kernel(const double* __restrict__ D, long long n,
                                                                const long long* __restrict__ node_ptr,
                                                                const int* __restrict__ members, long long n_members,
                                                                double* __restrict__ S) {
#pragma clang fp contract(off)
  const long long v = blockIdx.x;
  const long long i = (long long)blockIdx.y * SIL_THREADS + threadIdx.x;
  long long p = node_ptr[v], p1 = node_ptr[v + 1];
  p = p < 0 ? 0 : (p > n_members ? n_members : p);
  p1 = p1 < p ? p : (p1 > n_members ? n_members : p1);
  if (i >= n) return;
  double s = 0.0;
  for (; p + SIL_UNROLL <= p1; p += SIL_UNROLL) {
    double t[SIL_UNROLL];
#pragma unroll
    for (int u = 0; u < SIL_UNROLL; ++u) t[u] = dist_of<SQUARE>(D, n, i, members[p + u]);
#pragma unroll
    for (int u = 0; u < SIL_UNROLL; ++u) s = s + t[u];
  }
  for (; p < p1; ++p) s = s + dist_of<SQUARE>(D, n, i, members[p]);
  S[v * n + i] = s;
}

// samples[c, i] of cut c: a = S[own, i] / (|own| - 1), b = min over the cut's other nodes of
// S[v, i] / |v|, s = (b - a) / max(a, b), NaN -> +0.0.  True fp64 divisions.  One lane per (cut,
// point); the node index is uniform over the workgroup.  A node index outside [0, n_nodes) reads
// nothing: as `own` it gives s = +0.0, in the active list it is passed over.
__global__ __launch_bounds__(SIL_THREADS) void cut_samples_kernel(const double* __restrict__ S, long long n,
                                                                  long long n_nodes, const int* __restrict__ sizes,
                                                                  const long long* __restrict__ cut_ptr,
                                                                  const int* __restrict__ active, long long n_active,
                                                                  const int* __restrict__ own,
                                                                  double* __restrict__ samples) {
#pragma clang fp contract(off)
  const long long c = blockIdx.x;
  const long long i = (long long)blockIdx.y * SIL_THREADS + threadIdx.x;
  long long q = cut_ptr[c], q1 = cut_ptr[c + 1];
  q = q < 0 ? 0 : (q > n_active ? n_active : q);
  q1 = q1 < q ? q : (q1 > n_active ? n_active : q1);
  if (i >= n) return;
  const long long o = own[c * n + i];
  double a = __builtin_nan("");
  if (o >= 0 && o < n_nodes) a = S[o * n + i] / (double)(sizes[o] - 1);
  double b = __builtin_inf();
#pragma unroll 4
  for (; q < q1; ++q) {
    const long long v = active[q];
    if (v < 0 || v >= n_nodes || v == o) continue;
    const double t = S[v * n + i] / (double)sizes[v];
    b = t < b ? t : b;
  }
  const double m = a > b ? a : b;   // either order of a NaN a leaves s NaN: the numerator is NaN
  const double s = (b - a) / m;
  samples[c * n + i] = s != s ? 0.0 : s;
}

// offsets[0] = 0, non-decreasing, every part's length in [lo, hi]
bool csr_ok(const long long* ptr, long long parts, long long lo, long long hi) {
  if (ptr[0] != 0) return false;
  for (long long k = 0; k < parts; ++k) {
    const long long len = ptr[k + 1] - ptr[k];
    if (len < lo || len > hi) return false;
  }
  return true;
}

dim3 sil_grid(long long parts, long long n) {
  return dim3((unsigned)parts, (unsigned)((n + SIL_THREADS - 1) / SIL_THREADS));
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_square_distances(const double* condensed, long long n, double* square, void* stream) {
  EXPECTO_REQUIRE(n >= 2, "square_distances: fewer than 2 points");
  EXPECTO_REQUIRE(n <= SIL_MAX_N, "square_distances: at most 1048576 points per call");
  EXPECTO_REQUIRE(condensed && square, "null argument");
  const unsigned T = (unsigned)((n + SQ_TILE - 1) / SQ_TILE);
  square_distances_kernel<<<dim3(T, T), dim3(SIL_THREADS), 0, as_stream(stream)>>>(condensed, n, square);
  return check_launch("square_distances");
}

int expecto_silhouette_node_sums(const double* dist, int square, long long n, const long long* node_ptr_host,
                                 const long long* node_ptr, const int* members, long long n_nodes, double* S,
                                 void* stream) {
  EXPECTO_REQUIRE(n >= 2, "silhouette_node_sums: fewer than 2 points");
  EXPECTO_REQUIRE(n <= SIL_MAX_N, "silhouette_node_sums: at most 1048576 points per call");
  EXPECTO_REQUIRE(n_nodes >= 0 && n_nodes <= 0x7fffffffLL, "silhouette_node_sums: node count out of range");
  if (n_nodes == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(dist && node_ptr_host && node_ptr && members && S, "null argument");
  EXPECTO_REQUIRE(csr_ok(node_ptr_host, n_nodes, 0, n),
                  "silhouette_node_sums: inconsistent node offsets (first not 0, decreasing, or a node of more "
                  "than n members)");
  const long long n_members = node_ptr_host[n_nodes];
  if (square)
    node_sums_kernel<true><<<sil_grid(n_nodes, n), dim3(SIL_THREADS), 0, as_stream(stream)>>>(dist, n, node_ptr, members,
                                                                                              n_members, S);
  else
    node_sums_kernel<false><<<sil_grid(n_nodes, n), dim3(SIL_THREADS), 0, as_stream(stream)>>>(dist, n, node_ptr, members,
                                                                                               n_members, S);
  return check_launch("silhouette_node_sums");
}

int expecto_silhouette_cuts(const double* S, long long n, long long n_nodes, const int* sizes,
                            const long long* cut_ptr_host, const long long* cut_ptr, const int* active, const int* own,
                            long long n_cuts, double* samples, void* stream) {
  EXPECTO_REQUIRE(n >= 2, "silhouette_cuts: fewer than 2 points");
  EXPECTO_REQUIRE(n <= SIL_MAX_N, "silhouette_cuts: at most 1048576 points per call");
  EXPECTO_REQUIRE(n_nodes >= 0 && n_nodes <= 0x7fffffffLL && n_cuts >= 0 && n_cuts <= 0x7fffffffLL,
                  "silhouette_cuts: node or cut count out of range");
  if (n_cuts == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(S && sizes && cut_ptr_host && cut_ptr && active && own && samples, "null argument");
  EXPECTO_REQUIRE(cut_ptr_host[0] == 0, "silhouette_cuts: inconsistent cut offsets (first not 0)");
  EXPECTO_REQUIRE(csr_ok(cut_ptr_host, n_cuts, 2, n - 1),
                  "silhouette_cuts: a cut of fewer than 2 or more than n - 1 clusters (or inconsistent cut offsets)");
  EXPECTO_REQUIRE(n_nodes >= 2, "silhouette_cuts: a cut needs at least 2 nodes");
  cut_samples_kernel<<<sil_grid(n_cuts, n), dim3(SIL_THREADS), 0, as_stream(stream)>>>(
      S, n, n_nodes, sizes, cut_ptr, active, cut_ptr_host[n_cuts], own, samples);
  return check_launch("silhouette_cuts");
}

}  // extern "C"
