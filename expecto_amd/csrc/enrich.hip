// Motif-match enrichment of the top clusters (cluster_analysis_with_fimo.py:126-162) for a batch of
// problems over one contribution matrix, and the hypergeometric upper tail of the counts.
//
// enrich_prepare_kernel: what no problem changes.  hits[s, c] = the entries of sequence s whose motif is
// in column c's set, bits[c] = that set's popcount, and min_rank = C everywhere.
// enrich_kernel: one workgroup per (problem, block of EN_ROWS rows), one wave per row at a time.  The
// wave ranks the row's C magnitudes by counting (rank[c] = the columns that sort before c), which needs
// no sort network and makes ties exact: the lower column first.  pos_* of rank t are then lookups of
// hits / bits at order[t]; the bottom n_neg sets are OR-ed into LDS, counted, and the row's entries
// tested against the union.  Every sum is an integer, added with LDS atomics inside the workgroup and
// one global atomic per non-zero result: the result depends neither on the grid nor on the order.
// hypergeom_sf_kernel: one lane per quadruple.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"

namespace expecto {
namespace {

constexpr long long EN_MAX_C = 1024;
constexpr long long EN_MAX_M = 32768;        // 512 words of union bitset per wave
constexpr long long EN_MAX_P = 1LL << 20;
constexpr int EN_COLS = 4;                   // int64 columns of a problem row
enum { ENP_PERM = 0, ENP_SID = 1, ENP_ROW_OFF = 2, ENP_ROW_CNT = 3 };
constexpr int EN_ROWS = 32;                  // rows per workgroup
constexpr int EN_THREADS = 256;
constexpr size_t EN_LDS_LIMIT = 64 * 1024;

typedef unsigned long long u64;

__host__ __device__ inline size_t enrich_lds_bytes(int waves, int C, int W, int T) {
  // per wave: magnitudes, union words, order; per workgroup: two sums per rank, two bottom sums, least ranks
  return (size_t)waves * ((size_t)C * 8 + (size_t)W * 8 + (size_t)((C + 3) / 4) * 8) + (size_t)(2 * T + 2) * 8 +
         (size_t)C * 4;
}

__global__ __launch_bounds__(EN_THREADS) void enrich_prepare_kernel(
    const u64* __restrict__ sets, int C, int W, int M, const long long* __restrict__ seq_ptr,
    const int* __restrict__ motif_idx, long long S, long long nnz, long long P, int* __restrict__ hits,
    int* __restrict__ bits, int* __restrict__ min_rank) {
  const long long idx = (long long)blockIdx.x * EN_THREADS + threadIdx.x;
  if (idx < P * C) min_rank[idx] = C;
  if (idx < C) {
    int b = 0;
    for (int w = 0; w < W; ++w) b += __popcll(sets[(long long)idx * W + w]);
    bits[idx] = b;
  }
  if (idx < S * C) {
    const long long s = idx / C;
    const int c = (int)(idx % C);
    long long e0 = seq_ptr[s], e1 = seq_ptr[s + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > nnz) e1 = nnz;
    const u64* set = sets + (long long)c * W;
    int h = 0;
    for (long long e = e0; e < e1; ++e) {
      const int m = motif_idx[e];
      if (m >= 0 && m < M) h += (int)((set[m >> 6] >> (m & 63)) & 1ULL);
    }
    hits[idx] = h;
  }
}

__global__ __launch_bounds__(EN_THREADS) void enrich_kernel(
    const double* __restrict__ contrib, long long V, int C, long long ld, const u64* __restrict__ sets, int W, int M,
    const long long* __restrict__ seq_ptr, const int* __restrict__ motif_idx, long long S, long long nnz,
    const long long* __restrict__ prob, const unsigned short* __restrict__ perms, long long n_perms,
    const int* __restrict__ sids, long long n_sids, const int* __restrict__ rows, long long rows_len, int n_neg, int T,
    const int* __restrict__ hits, const int* __restrict__ bits, u64* __restrict__ pos_matches,
    u64* __restrict__ pos_motifs, u64* __restrict__ neg, int* __restrict__ min_rank) {
  extern __shared__ __attribute__((aligned(16))) unsigned char en_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const long long p = blockIdx.x;
  const long long* pr = prob + p * EN_COLS;
  const long long perm_slot = pr[ENP_PERM], sid_slot = pr[ENP_SID], row_off = pr[ENP_ROW_OFF], row_cnt = pr[ENP_ROW_CNT];
  // the device copy of the table is not the one the host checked: a row that does not fit is passed over
  if (perm_slot < -1 || perm_slot >= n_perms || sid_slot < 0 || sid_slot >= n_sids || row_off < 0 || row_cnt < 0 ||
      row_off + row_cnt > rows_len)
    return;
  const long long r0 = (long long)blockIdx.y * EN_ROWS;
  if (r0 >= row_cnt) return;

  double* mag_all = reinterpret_cast<double*>(en_lds);
  u64* uni_all = reinterpret_cast<u64*>(mag_all + (size_t)waves * C);
  unsigned short* ord_all = reinterpret_cast<unsigned short*>(uni_all + (size_t)waves * W);
  const int ord_stride = ((C + 3) / 4) * 4;
  u64* acc_m = reinterpret_cast<u64*>(ord_all + (size_t)waves * ord_stride);     // pos_matches [T]
  u64* acc_b = acc_m + T;                                                           // pos_motifs [T]
  u64* acc_neg = acc_b + T;                                                         // neg_matches, neg_motifs
  int* least = reinterpret_cast<int*>(acc_neg + 2);                                // [C]
  double* mag = mag_all + (size_t)wave * C;
  u64* uni = uni_all + (size_t)wave * W;
  unsigned short* ord = ord_all + (size_t)wave * ord_stride;

  for (int i = tid; i < 2 * T + 2; i += blockDim.x) acc_m[i] = 0;
  for (int i = tid; i < C; i += blockDim.x) least[i] = C;
  __syncthreads();

  const unsigned short* perm = perm_slot >= 0 ? perms + perm_slot * V * C : nullptr;
  const int* sid_map = sids + sid_slot * V;

  for (int it = 0; it < EN_ROWS; it += waves) {      // the same trip count in every wave: barriers inside
    const long long r = r0 + it + wave;
    long long v = -1;
    if (r < row_cnt) {
      v = rows[row_off + r];
      if (v < 0 || v >= V) v = -1;
    }
    const bool live = v >= 0;
    long long e0 = 0, e1 = 0;
    if (live) {
      const int s = sid_map[v];
      if (s >= 0 && s < S) {
        e0 = seq_ptr[s];
        e1 = seq_ptr[s + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > nnz) e1 = nnz;
      }
      for (int c = lane; c < C; c += 64) {
        int col = perm ? (int)perm[v * C + c] : c;
        if (col >= C) col = c;
        mag[c] = fabs(contrib[v * ld + col]);
      }
    }
    __syncthreads();
    if (live) {
      for (int c = lane; c < C; c += 64) {
        const double a = mag[c];
        int rank = 0;
        for (int j = 0; j < C; ++j) {
          const double b = mag[j];
          rank += (b > a || (b == a && j < c)) ? 1 : 0;
        }
        ord[rank] = (unsigned short)c;
        atomicMin(&least[c], rank);
      }
    }
    __syncthreads();
    if (live) {
      const int s = sid_map[v];
      const int* hrow = (s >= 0 && s < S) ? hits + (long long)s * C : nullptr;
      for (int t = lane; t < T; t += 64) {
        const int c = ord[t];
        if (hrow) {
          const int h = hrow[c];
          if (h) atomicAdd(&acc_m[t], (u64)h);
        }
        atomicAdd(&acc_b[t], (u64)bits[c]);
      }
      int nb = 0;
      for (int w = lane; w < W; w += 64) {
        u64 u = 0;
        for (int q = C - n_neg; q < C; ++q) u |= sets[(long long)ord[q] * W + w];
        uni[w] = u;
        nb += __popcll(u);
      }
      if (nb) atomicAdd(&acc_neg[1], (u64)nb);
    }
    __syncthreads();
    if (live) {
      int nm = 0;
      for (long long e = e0 + lane; e < e1; e += 64) {
        const int m = motif_idx[e];
        if (m >= 0 && m < M) nm += (int)((uni[m >> 6] >> (m & 63)) & 1ULL);
      }
      if (nm) atomicAdd(&acc_neg[0], (u64)nm);
    }
    // the next row's magnitudes, order and union are each written after a later barrier than their last read
  }
  __syncthreads();
  for (int t = tid; t < T; t += blockDim.x) {
    if (acc_m[t]) atomicAdd(&pos_matches[p * T + t], acc_m[t]);
    if (acc_b[t]) atomicAdd(&pos_motifs[p * T + t], acc_b[t]);
  }
  if (tid < 2 && acc_neg[tid]) atomicAdd(&neg[p * 2 + tid], acc_neg[tid]);
  for (int c = tid; c < C; c += blockDim.x)
    if (least[c] < C) atomicMin(&min_rank[p * C + c], least[c]);
}

// The hypergeometric mass at i, C(n, i) C(M - n, N - i) / C(M, N), as a product of its 2 min(n, N) integer
// ratios with the exponent kept apart.  Differences of lgamma lose eps * lgamma(M) absolutely, 1e-9 of
// the result at M = 1e6; here every factor is rounded twice, about 1e-13 after 2e5 factors.
__device__ double hypergeom_pmf(long long i, long long M, long long n, long long N) {
  if (N > n) { const long long t = n; n = N; N = t; }      // symmetric in n and N: the shorter products
  double m = 1.0;
  int ex = 0;
  auto mul = [&](long long num, long long den) {
    m = m * ((double)num / (double)den);
    if (m > 0x1p500 || m < 0x1p-500) {
      int e;
      m = frexp(m, &e);
      ex += e;
    }
  };
  for (long long j = 1; j <= i; ++j) mul(n - i + j, j);
  for (long long j = 1; j <= N - i; ++j) mul(M - n - N + i + j, j);
  for (long long j = 1; j <= N; ++j) mul(j, M - N + j);
  return ldexp(m, ex);
}

__global__ __launch_bounds__(256) void hypergeom_sf_kernel(const long long* __restrict__ k_, const long long* __restrict__ M_,
                                                           const long long* __restrict__ n_, const long long* __restrict__ N_,
                                                           long long count, double* __restrict__ out) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= count) return;
  const long long k = k_[q], M = M_[q], n = n_[q], N = N_[q];
  if (M <= 0 || n < 0 || N < 0 || n > M || N > M) {   // scipy's argument check
    out[q] = __builtin_nan("");
    return;
  }
  const long long lo = N - (M - n) > 0 ? N - (M - n) : 0, hi = n < N ? n : N;
  if (k <= lo) { out[q] = 1.0; return; }
  if (k > hi) { out[q] = 0.0; return; }
  // the terms rise to the mode and fall after it: start at the tail's largest term, so that the first
  // term cannot underflow under a tail that does not, and every other term is a ratio times its neighbour
  long long start = (long long)(((double)(n + 1) * (double)(N + 1)) / (double)(M + 2));
  if (start < k) start = k;
  if (start > hi) start = hi;
  const double Md = (double)M, nd = (double)n, Nd = (double)N;
  const double first = hypergeom_pmf(start, M, n, N);
  double sum = first, term = first;
  for (long long i = start; i < hi; ++i) {
    const double x = (double)i;
    term = term * ((nd - x) * (Nd - x)) / ((x + 1.0) * (Md - nd - Nd + x + 1.0));
    const double s = sum + term;
    if (s == sum) break;
    sum = s;
  }
  term = first;
  for (long long i = start; i > k; --i) {
    const double x = (double)i;
    term = term * (x * (Md - nd - Nd + x)) / ((nd - x + 1.0) * (Nd - x + 1.0));
    const double s = sum + term;
    if (s == sum) break;
    sum = s;
  }
  out[q] = sum < 1.0 ? sum : 1.0;
}

size_t enrich_workspace_bytes(long long S, long long C) {
  if (S < 0 || C < 1 || C > EN_MAX_C || S > (1LL << 31) / C) return 0;
  return (size_t)(S * C + C) * 4;
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

size_t expecto_cluster_enrich_workspace(long long S, long long C) { return enrich_workspace_bytes(S, C); }

int expecto_cluster_enrich(const double* contrib, long long V, long long C, long long ld,
                           const unsigned long long* sets, long long M, const long long* seq_ptr_host,
                           const long long* seq_ptr, const int* motif_idx, long long S, const long long* prob_host,
                           const long long* prob, long long P, const unsigned short* perms, long long n_perms,
                           const int* sids, long long n_sids, const int* rows, long long rows_len, long long n_neg,
                           long long T, long long* pos_matches, long long* pos_motifs, long long* neg, int* min_rank,
                           void* workspace, size_t workspace_bytes, void* stream) {
  EXPECTO_REQUIRE(V >= 0 && P >= 0 && S >= 0 && n_perms >= 0 && n_sids >= 0 && rows_len >= 0,
                  "cluster_enrich: negative count");
  EXPECTO_REQUIRE(P <= EN_MAX_P, "cluster_enrich: problem count out of range (at most 1048576)");
  EXPECTO_REQUIRE(C >= 1 && C <= EN_MAX_C, "cluster_enrich: C must lie in [1, 1024]");
  EXPECTO_REQUIRE(ld >= C, "cluster_enrich: row stride ld < C");
  EXPECTO_REQUIRE(M >= 1 && M <= EN_MAX_M, "cluster_enrich: M must lie in [1, 32768]");
  EXPECTO_REQUIRE(n_neg >= 1 && n_neg <= C, "cluster_enrich: n_neg must lie in [1, C]");
  EXPECTO_REQUIRE(T >= 1 && T <= C, "cluster_enrich: T must lie in [1, C]");
  EXPECTO_REQUIRE(V <= (1LL << 31) / C && S <= (1LL << 31) / C, "cluster_enrich: V * C and S * C must stay below 2^31");
  if (P == 0 || V == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(contrib && sets && seq_ptr_host && seq_ptr && prob_host && prob && sids && rows && pos_matches &&
                      pos_motifs && neg && min_rank && workspace,
                  "null argument");
  EXPECTO_REQUIRE(n_sids >= 1, "cluster_enrich: no sid map");
  EXPECTO_REQUIRE(seq_ptr_host[0] == 0, "cluster_enrich: seq_ptr[0] != 0");
  for (long long s = 0; s < S; ++s)
    EXPECTO_REQUIRE(seq_ptr_host[s + 1] >= seq_ptr_host[s], "cluster_enrich: decreasing seq_ptr");
  const long long nnz = seq_ptr_host[S];
  EXPECTO_REQUIRE(nnz == 0 || motif_idx, "null argument");
  long long max_rows = 0;
  for (long long p = 0; p < P; ++p) {
    const long long* r = prob_host + p * EN_COLS;
    EXPECTO_REQUIRE(r[ENP_PERM] >= -1 && r[ENP_PERM] < n_perms, "cluster_enrich: permutation slot out of range");
    EXPECTO_REQUIRE(r[ENP_PERM] < 0 || perms, "null argument");
    EXPECTO_REQUIRE(r[ENP_SID] >= 0 && r[ENP_SID] < n_sids, "cluster_enrich: sid slot out of range");
    EXPECTO_REQUIRE(r[ENP_ROW_OFF] >= 0 && r[ENP_ROW_CNT] >= 0 && r[ENP_ROW_OFF] + r[ENP_ROW_CNT] <= rows_len,
                    "cluster_enrich: row list outside rows");
    if (r[ENP_ROW_CNT] > max_rows) max_rows = r[ENP_ROW_CNT];
  }
  EXPECTO_REQUIRE(max_rows <= 65535LL * EN_ROWS, "cluster_enrich: at most 2097120 rows per problem");
  const size_t need = enrich_workspace_bytes(S, C);
  EXPECTO_REQUIRE(need && workspace_bytes >= need, "cluster_enrich: workspace too small (expecto_cluster_enrich_workspace)");
  EXPECTO_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "cluster_enrich: workspace not 4-byte aligned");

  hipStream_t st = as_stream(stream);
  {   // the one host read of contrib: a NaN has no rank
    std::vector<double> host((size_t)((V - 1) * ld + C));
    EXPECTO_HIP_CHECK(hipMemcpyAsync(host.data(), contrib, host.size() * 8, hipMemcpyDeviceToHost, st));
    EXPECTO_HIP_CHECK(hipStreamSynchronize(st));
    for (long long v = 0; v < V; ++v)
      for (long long c = 0; c < C; ++c)
        EXPECTO_REQUIRE(!std::isnan(host[(size_t)(v * ld + c)]), "cluster_enrich: NaN in contrib");
  }

  const int W = (int)((M + 63) / 64);
  int* hits = static_cast<int*>(workspace);
  int* bits = hits + S * C;
  EXPECTO_HIP_CHECK(hipMemsetAsync(pos_matches, 0, (size_t)(P * T) * 8, st));
  EXPECTO_HIP_CHECK(hipMemsetAsync(pos_motifs, 0, (size_t)(P * T) * 8, st));
  EXPECTO_HIP_CHECK(hipMemsetAsync(neg, 0, (size_t)(P * 2) * 8, st));
  long long prep = S * C > P * C ? S * C : P * C;
  enrich_prepare_kernel<<<dim3((unsigned)((prep + EN_THREADS - 1) / EN_THREADS)), dim3(EN_THREADS), 0, st>>>(
      sets, (int)C, W, (int)M, seq_ptr, motif_idx, S, nnz, P, hits, bits, min_rank);
  if (int e = check_launch("cluster_enrich (prepare)")) return e;
  if (max_rows == 0) return EXPECTO_OK;
  int waves = EN_THREADS / 64;
  while (waves > 1 && enrich_lds_bytes(waves, (int)C, W, (int)T) > EN_LDS_LIMIT) waves /= 2;
  const size_t lds = enrich_lds_bytes(waves, (int)C, W, (int)T);
  EXPECTO_REQUIRE(lds <= EN_LDS_LIMIT, "cluster_enrich: C, M and T need more than 64 KiB of LDS");
  enrich_kernel<<<dim3((unsigned)P, (unsigned)((max_rows + EN_ROWS - 1) / EN_ROWS)), dim3(64 * waves), lds, st>>>(
      contrib, V, (int)C, ld, sets, W, (int)M, seq_ptr, motif_idx, S, nnz, prob, perms, n_perms, sids, n_sids, rows,
      rows_len, (int)n_neg, (int)T, hits, bits, reinterpret_cast<u64*>(pos_matches), reinterpret_cast<u64*>(pos_motifs),
      reinterpret_cast<u64*>(neg), min_rank);
  return check_launch("cluster_enrich");
}

int expecto_hypergeom_sf(const long long* k, const long long* M, const long long* n, const long long* N,
                         long long count, double* out, void* stream) {
  EXPECTO_REQUIRE(count >= 0, "hypergeom_sf: negative count");
  if (count == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(k && M && n && N && out, "null argument");
  hypergeom_sf_kernel<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(k, M, n, N, count, out);
  return check_launch("hypergeom_sf");
}

}  // extern "C"
