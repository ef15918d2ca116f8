// Truncated SVD of the tf-idf mark tracks (svd.py, svd_transform.py): the column statistics, the
// float64 Gram matrix of the tf-idf rows (fp64 MFMA), the projection that gives components_ and the
// transform of a track matrix by them.  The eigenproblem of the Gram matrix stays on the host.
//
// Every kernel reads one chunk of columns D [n, ld] float32 as the per-gene files hold it (marks
// contiguous), gathers the kept marks through keep_idx and forms t[n,i] = x[n,i] * idf_n in float64
// while it stages a panel into LDS.  No atomics: every sum has a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "common.h"
#include "tri_tiles.h"

namespace expecto {
namespace {

constexpr int TG_TILE = 64;       // a workgroup's tile of the output: TG_TILE x TG_TILE
constexpr int TG_KS = 32;         // columns (or, in the projection, marks) staged through LDS at a time
constexpr int TG_THREADS = 256;
constexpr int TG_LDW = TG_TILE + 16;   // Gram panels [TG_KS][TG_LDW] doubles: rows k and k+1 of one MFMA operand
                                       // read (16 lanes each) land in opposite halves of the 64 banks
constexpr int TG_LDP = TG_KS + 1;      // projection panels [TG_TILE][TG_LDP]: 16 rows' reads of one k hit 32 banks
constexpr int TG_LDV = TG_TILE + 1;    // transform's component panel [TG_KS][TG_LDV]: 32 columns' stores spread
constexpr long long TG_TARGET_WGS = 4096;   // split the columns until tiles x parts reaches this
constexpr long long TG_MAX_PARTS = 64;
constexpr long long TG_MAX_M = 1LL << 20;   // tile counts stay far below 2^31
constexpr int RS_MARKS = 16, RS_ROWS = 16;  // row sums: 16 marks x 16 interleaved column lanes per workgroup

typedef double double4_t __attribute__((ext_vector_type(4)));

// Columns per part (a multiple of TG_KS) and the number of parts for `tiles` output tiles.
inline long long split_columns(long long tiles, long long n, long long* part_len) {
  const long long stages = (n + TG_KS - 1) / TG_KS;
  long long want = (TG_TARGET_WGS + tiles - 1) / tiles;
  if (want > TG_MAX_PARTS) want = TG_MAX_PARTS;
  if (want > stages) want = stages;
  if (want < 1) want = 1;
  const long long per = (stages + want - 1) / want;
  *part_len = per * TG_KS;
  return (stages + per - 1) / per;
}

inline long long gram_tiles(long long m) {
  const long long T = (m + TG_TILE - 1) / TG_TILE;
  return T * (T + 1) / 2;
}

inline long long transform_tiles(long long m, long long k) {
  return ((m + TG_TILE - 1) / TG_TILE) * ((k + TG_TILE - 1) / TG_TILE);
}

// idf[n] = log(m / (1 + sum_i x[n, i])), the sum in float64 over i ascending: one lane per column.
__global__ __launch_bounds__(TG_THREADS) void tfidf_idf_kernel(const float* __restrict__ D, long long n, long long ld,
                                                               const int* __restrict__ keep, int m,
                                                               double* __restrict__ idf) {
  const long long nn = (long long)blockIdx.x * TG_THREADS + threadIdx.x;
  if (nn >= n) return;
  const float* row = D + nn * ld;
  double s = 0.0;
  for (int i = 0; i < m; ++i) s = s + (double)row[keep[i]];
  idf[nn] = log((double)m / (1.0 + s));
}

// rowsum[i] += sum_n x[n, i].  A workgroup owns RS_MARKS marks; lane (mark, y) adds the columns
// y, y + 16, ... in ascending order, then the 16 partial sums of a mark are added in ascending y.
__global__ __launch_bounds__(RS_MARKS * RS_ROWS) void tfidf_rowsum_kernel(const float* __restrict__ D, long long n,
                                                                          long long ld, const int* __restrict__ keep,
                                                                          int m, double* __restrict__ rowsum) {
  __shared__ double part[RS_ROWS][RS_MARKS + 1];
  const int tx = threadIdx.x & (RS_MARKS - 1), ty = threadIdx.x / RS_MARKS;
  const int i = blockIdx.x * RS_MARKS + tx;
  double s = 0.0;
  if (i < m) {
    const float* col = D + keep[i];
#pragma unroll 8
    for (long long nn = ty; nn < n; nn += RS_ROWS) s = s + (double)col[nn * ld];
  }
  part[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && i < m) {
    double total = part[0][tx];
#pragma unroll
    for (int y = 1; y < RS_ROWS; ++y) total = total + part[y][tx];
    rowsum[i] = rowsum[i] + total;
  }
}

// One part of one upper-triangle tile of H = sum_n t[n,:]^T t[n,:]: the sum over the part's columns
// n0 .. n1-1 in ascending order, written whole (64 x 64, zero outside m) to the workspace.
//
// The two panels (tile rows bi, bj) are staged [column][mark] as float64 t values.  Wave w owns the
// 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 blocks of v_mfma_f64_16x16x4_f64; A and B both take
// (row or col = lane & 15, k = lane >> 4), the result register r of a lane is row (lane >> 4) + 4 r,
// column lane & 15.  A diagonal tile stages one panel and uses it for both operands.
__global__ __launch_bounds__(TG_THREADS) void tfidf_gram_parts_kernel(const float* __restrict__ D, long long n,
                                                                      long long ld, const int* __restrict__ keep,
                                                                      int m, const double* __restrict__ idf,
                                                                      double* __restrict__ ws, long long T,
                                                                      long long part_len) {
  __shared__ double As[TG_KS * TG_LDW];
  __shared__ double Bs[TG_KS * TG_LDW];
  int bi, bj;
  pd_tile_of(blockIdx.x, T, bi, bj);
  const bool diag = bi == bj;
  const long long n0 = (long long)blockIdx.y * part_len;
  const long long n1 = n0 + part_len < n ? n0 + part_len : n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;   // loads: mark `lane`, columns wave + 4 q
  const long long ia = (long long)bi * TG_TILE + lane, ib = (long long)bj * TG_TILE + lane;
  const long long ca = ia < m ? keep[ia] : -1;
  const long long cb = (!diag && ib < m) ? keep[ib] : -1;

  float ra[8], rb[8];
  double rw[8];
  auto fetch = [&](long long k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long nn = k0 + wave + 4 * q;
      const bool ok = nn < n1;
      rw[q] = ok ? idf[nn] : 0.0;
      ra[q] = (ok && ca >= 0) ? D[nn * ld + ca] : 0.0f;
      rb[q] = (ok && cb >= 0) ? D[nn * ld + cb] : 0.0f;
    }
  };

  double4_t acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[r][c] = double4_t{0.0, 0.0, 0.0, 0.0};

  const double* Bp = diag ? As : Bs;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int arow = 32 * (wave >> 1) + l15, bcol = 32 * (wave & 1) + l15;

  fetch(n0);
  for (long long k0 = n0; k0 < n1; k0 += TG_KS) {
    __syncthreads();   // the previous stage has been read
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      As[(wave + 4 * q) * TG_LDW + lane] = (double)ra[q] * rw[q];
      if (!diag) Bs[(wave + 4 * q) * TG_LDW + lane] = (double)rb[q] * rw[q];
    }
    __syncthreads();
    if (k0 + TG_KS < n1) fetch(k0 + TG_KS);   // the next stage's loads fly under this stage's MFMAs
#pragma unroll
    for (int kk = 0; kk < TG_KS / 4; ++kk) {
      const int k = 4 * kk + l4;
      const double a0 = As[k * TG_LDW + arow], a1 = As[k * TG_LDW + arow + 16];
      const double b0 = Bp[k * TG_LDW + bcol], b1 = Bp[k * TG_LDW + bcol + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  double* tile = ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (TG_TILE * TG_TILE);
#pragma unroll
  for (int rb2 = 0; rb2 < 2; ++rb2)
#pragma unroll
    for (int cb2 = 0; cb2 < 2; ++cb2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 32 * (wave >> 1) + 16 * rb2 + l4 + 4 * r;
        const int col = 32 * (wave & 1) + 16 * cb2 + l15;
        tile[row * TG_TILE + col] = acc[rb2][cb2][r];
      }
}

// H[i,j] (and H[j,i]) += the tile's parts added in ascending order.  A diagonal tile takes its
// entries j >= i only, so both triangles receive the same bits.
__global__ __launch_bounds__(TG_THREADS) void tfidf_gram_reduce_kernel(const double* __restrict__ ws, int parts,
                                                                       long long tiles, double* __restrict__ H, int m,
                                                                       long long T) {
  int bi, bj;
  pd_tile_of(blockIdx.x, T, bi, bj);
  const double* tile = ws + (long long)blockIdx.x * (TG_TILE * TG_TILE);
  for (int e = threadIdx.x; e < TG_TILE * TG_TILE; e += TG_THREADS) {
    const long long i = (long long)bi * TG_TILE + e / TG_TILE, j = (long long)bj * TG_TILE + e % TG_TILE;
    if (i >= m || j >= m || j < i) continue;
    double s = tile[e];
    for (int p = 1; p < parts; ++p) s = s + tile[(long long)p * tiles * (TG_TILE * TG_TILE) + e];
    H[i * m + j] = H[i * m + j] + s;
    if (j != i) H[j * m + i] = H[j * m + i] + s;
  }
}

// out[c, n] = (float)(idf_n * sum_i P[c,i] x[n,i]): a 64-column x 64-component tile per workgroup,
// the marks staged TG_KS at a time in ascending order, a 4 x 4 micro-tile per lane.
__global__ __launch_bounds__(TG_THREADS) void tfidf_project_kernel(const float* __restrict__ D, long long n,
                                                                   long long ld, const int* __restrict__ keep, int m,
                                                                   const double* __restrict__ idf,
                                                                   const double* __restrict__ Pm, int k,
                                                                   float* __restrict__ out, long long ld_out) {
  __shared__ double Xs[TG_TILE * TG_LDP];
  __shared__ double Ps[TG_TILE * TG_LDP];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;   // columns nb + tx + 16 r  x  components cb + ty + 16 s
  const int lk = tid & 31, lp = tid >> 5;   // loads: mark lk of columns / components lp + 8 q
  const long long nb = (long long)blockIdx.x * TG_TILE;
  const int cb = blockIdx.y * TG_TILE;

  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = 0.0;

  float rx[8];
  double rp[8];
  auto fetch = [&](int i0) {
    const int i = i0 + lk;
    const long long col = i < m ? keep[i] : -1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long nn = nb + lp + 8 * q;
      const int c = cb + lp + 8 * q;
      rx[q] = (col >= 0 && nn < n) ? D[nn * ld + col] : 0.0f;
      rp[q] = (i < m && c < k) ? Pm[(long long)c * m + i] : 0.0;
    }
  };
  fetch(0);
  for (int i0 = 0; i0 < m; i0 += TG_KS) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      Xs[(lp + 8 * q) * TG_LDP + lk] = (double)rx[q];
      Ps[(lp + 8 * q) * TG_LDP + lk] = rp[q];
    }
    __syncthreads();
    if (i0 + TG_KS < m) fetch(i0 + TG_KS);
#pragma unroll 8
    for (int kk = 0; kk < TG_KS; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[r] = Xs[(tx + 16 * r) * TG_LDP + kk];
        b[r] = Ps[(ty + 16 * r) * TG_LDP + kk];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = __builtin_fma(a[r], b[s], acc[r][s]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long nn = nb + tx + 16 * r;
    if (nn >= n) continue;
    const double w = idf[nn];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = cb + ty + 16 * s;
      if (c < k) out[(long long)c * ld_out + nn] = (float)(w * acc[r][s]);
    }
  }
}

// One part of one 64-mark x 64-component tile of X[i,c] = sum_n x[n,i] idf_n V[c,n], the part's
// columns in ascending order, written whole to the workspace.
__global__ __launch_bounds__(TG_THREADS) void tfidf_transform_parts_kernel(
    const float* __restrict__ D, long long n, long long ld, const int* __restrict__ keep, int m,
    const double* __restrict__ idf, const float* __restrict__ V, long long ld_v, int k, double* __restrict__ ws,
    int tiles_k, long long part_len) {
  __shared__ double Xs[TG_KS * TG_TILE];
  __shared__ double Vs[TG_KS * TG_LDV];
  const int bm = blockIdx.x / tiles_k, bc = blockIdx.x % tiles_k;
  const long long n0 = (long long)blockIdx.y * part_len;
  const long long n1 = n0 + part_len < n ? n0 + part_len : n;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;   // track loads: mark `lane`, columns wave + 4 q
  const int lk = tid & 31, lp = tid >> 5;       // component loads: column lk, components lp + 8 q
  const int tx = tid & 15, ty = tid >> 4;       // marks ty + 16 r  x  components tx + 16 s
  const long long im = (long long)bm * TG_TILE + lane;
  const long long col = im < m ? keep[im] : -1;

  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = 0.0;

  float rx[8], rv[8];
  double rw[8];
  auto fetch = [&](long long k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long nn = k0 + wave + 4 * q;
      const bool ok = nn < n1;
      rw[q] = ok ? idf[nn] : 0.0;
      rx[q] = (ok && col >= 0) ? D[nn * ld + col] : 0.0f;
      const long long nv = k0 + lk;
      const int c = bc * TG_TILE + lp + 8 * q;
      rv[q] = (nv < n1 && c < k) ? V[(long long)c * ld_v + nv] : 0.0f;
    }
  };
  fetch(n0);
  for (long long k0 = n0; k0 < n1; k0 += TG_KS) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      Xs[(wave + 4 * q) * TG_TILE + lane] = (double)rx[q] * rw[q];
      Vs[lk * TG_LDV + lp + 8 * q] = (double)rv[q];
    }
    __syncthreads();
    if (k0 + TG_KS < n1) fetch(k0 + TG_KS);
#pragma unroll 8
    for (int kk = 0; kk < TG_KS; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[r] = Xs[kk * TG_TILE + ty + 16 * r];
        b[r] = Vs[kk * TG_LDV + tx + 16 * r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = __builtin_fma(a[r], b[s], acc[r][s]);
    }
  }
  double* tile = ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (TG_TILE * TG_TILE);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) tile[(ty + 16 * r) * TG_TILE + tx + 16 * s] = acc[r][s];
}

// X[i,c] += the tile's parts added in ascending order.
__global__ __launch_bounds__(TG_THREADS) void tfidf_transform_reduce_kernel(const double* __restrict__ ws, int parts,
                                                                            long long tiles, double* __restrict__ X,
                                                                            int m, int k, int tiles_k) {
  const int bm = blockIdx.x / tiles_k, bc = blockIdx.x % tiles_k;
  const double* tile = ws + (long long)blockIdx.x * (TG_TILE * TG_TILE);
  for (int e = threadIdx.x; e < TG_TILE * TG_TILE; e += TG_THREADS) {
    const long long i = (long long)bm * TG_TILE + e / TG_TILE;
    const int c = bc * TG_TILE + e % TG_TILE;
    if (i >= m || c >= k) continue;
    double s = tile[e];
    for (int p = 1; p < parts; ++p) s = s + tile[(long long)p * tiles * (TG_TILE * TG_TILE) + e];
    X[i * k + c] = X[i * k + c] + s;
  }
}

}  // namespace
}  // namespace expecto

using namespace expecto;

#define TFIDF_COMMON_CHECKS(what)                                                            \
  EXPECTO_REQUIRE(n >= 0 && m >= 0, what ": negative shape");                                \
  EXPECTO_REQUIRE(m <= TG_MAX_M, what ": at most 1048576 kept marks");                       \
  EXPECTO_REQUIRE(ld >= m, what ": row stride ld < m (ld must exceed every keep_idx entry)")

extern "C" {

int expecto_tfidf_stats(const float* D, long long n, long long ld, const int* keep_idx, int m, double* idf,
                        double* rowsum_acc, void* stream) {
  TFIDF_COMMON_CHECKS("tfidf_stats");
  if (n == 0 || m == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(D && keep_idx && idf && rowsum_acc, "null argument");
  tfidf_idf_kernel<<<dim3((unsigned)((n + TG_THREADS - 1) / TG_THREADS)), dim3(TG_THREADS), 0, as_stream(stream)>>>(
      D, n, ld, keep_idx, m, idf);
  tfidf_rowsum_kernel<<<dim3((unsigned)((m + RS_MARKS - 1) / RS_MARKS)), dim3(RS_MARKS * RS_ROWS), 0,
                        as_stream(stream)>>>(D, n, ld, keep_idx, m, rowsum_acc);
  return check_launch("tfidf_stats");
}

int expecto_tfidf_gram_parts(int m, long long n) {
  if (m <= 0 || n <= 0 || m > TG_MAX_M) return 0;
  long long len;
  return (int)split_columns(gram_tiles(m), n, &len);
}

size_t expecto_tfidf_gram_workspace(int m, long long n) {
  if (m <= 0 || n <= 0 || m > TG_MAX_M) return 0;
  long long len;
  return (size_t)(split_columns(gram_tiles(m), n, &len) * gram_tiles(m)) * TG_TILE * TG_TILE * sizeof(double);
}

int expecto_tfidf_gram(const float* D, long long n, long long ld, const int* keep_idx, int m, const double* idf,
                       double* H_acc, void* workspace, size_t workspace_bytes, void* stream) {
  TFIDF_COMMON_CHECKS("tfidf_gram");
  if (n == 0 || m == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(D && keep_idx && idf && H_acc && workspace, "null argument");
  EXPECTO_REQUIRE(workspace_bytes >= expecto_tfidf_gram_workspace(m, n),
                  "tfidf_gram: workspace smaller than expecto_tfidf_gram_workspace(m, n)");
  const long long T = (m + TG_TILE - 1) / TG_TILE, tiles = gram_tiles(m);
  long long len;
  const long long parts = split_columns(tiles, n, &len);
  tfidf_gram_parts_kernel<<<dim3((unsigned)tiles, (unsigned)parts), dim3(TG_THREADS), 0, as_stream(stream)>>>(
      D, n, ld, keep_idx, m, idf, (double*)workspace, T, len);
  tfidf_gram_reduce_kernel<<<dim3((unsigned)tiles), dim3(TG_THREADS), 0, as_stream(stream)>>>(
      (const double*)workspace, (int)parts, tiles, H_acc, m, T);
  return check_launch("tfidf_gram");
}

int expecto_tfidf_project(const float* D, long long n, long long ld, const int* keep_idx, int m, const double* idf,
                          const double* P, int k, float* out, long long ld_out, void* stream) {
  TFIDF_COMMON_CHECKS("tfidf_project");
  EXPECTO_REQUIRE(k >= 0, "tfidf_project: negative shape");
  EXPECTO_REQUIRE(k <= 65535 * TG_TILE, "tfidf_project: at most 4194240 components");
  EXPECTO_REQUIRE(ld_out >= n, "tfidf_project: row stride ld_out < n");
  if (n == 0 || m == 0 || k == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(D && keep_idx && idf && P && out, "null argument");
  tfidf_project_kernel<<<dim3((unsigned)((n + TG_TILE - 1) / TG_TILE), (unsigned)((k + TG_TILE - 1) / TG_TILE)),
                         dim3(TG_THREADS), 0, as_stream(stream)>>>(D, n, ld, keep_idx, m, idf, P, k, out, ld_out);
  return check_launch("tfidf_project");
}

int expecto_tfidf_transform_parts(int m, int k, long long n) {
  if (m <= 0 || k <= 0 || n <= 0 || m > TG_MAX_M) return 0;
  long long len;
  return (int)split_columns(transform_tiles(m, k), n, &len);
}

size_t expecto_tfidf_transform_workspace(int m, int k, long long n) {
  if (m <= 0 || k <= 0 || n <= 0 || m > TG_MAX_M) return 0;
  long long len;
  const long long tiles = transform_tiles(m, k);
  return (size_t)(split_columns(tiles, n, &len) * tiles) * TG_TILE * TG_TILE * sizeof(double);
}

int expecto_tfidf_transform(const float* D, long long n, long long ld, const int* keep_idx, int m, const double* idf,
                            const float* V, long long ld_v, int k, double* X_acc, void* workspace,
                            size_t workspace_bytes, void* stream) {
  TFIDF_COMMON_CHECKS("tfidf_transform");
  EXPECTO_REQUIRE(k >= 0, "tfidf_transform: negative shape");
  EXPECTO_REQUIRE(k <= TG_MAX_M, "tfidf_transform: at most 1048576 components");
  EXPECTO_REQUIRE(ld_v >= n, "tfidf_transform: row stride ld_v < n");
  if (n == 0 || m == 0 || k == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(D && keep_idx && idf && V && X_acc && workspace, "null argument");
  EXPECTO_REQUIRE(workspace_bytes >= expecto_tfidf_transform_workspace(m, k, n),
                  "tfidf_transform: workspace smaller than expecto_tfidf_transform_workspace(m, k, n)");
  const long long tiles = transform_tiles(m, k);
  EXPECTO_REQUIRE(tiles < (1LL << 31), "tfidf_transform: m x k too large");
  const int tiles_k = (k + TG_TILE - 1) / TG_TILE;
  long long len;
  const long long parts = split_columns(tiles, n, &len);
  tfidf_transform_parts_kernel<<<dim3((unsigned)tiles, (unsigned)parts), dim3(TG_THREADS), 0, as_stream(stream)>>>(
      D, n, ld, keep_idx, m, idf, V, ld_v, k, (double*)workspace, tiles_k, len);
  tfidf_transform_reduce_kernel<<<dim3((unsigned)tiles), dim3(TG_THREADS), 0, as_stream(stream)>>>(
      (const double*)workspace, (int)parts, tiles, X_acc, m, k, tiles_k);
  return check_launch("tfidf_transform");
}

}  // extern "C"
