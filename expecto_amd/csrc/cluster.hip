// Ward clustering of chromatin marks (interpret_features.py, interpret_features_grouped.py): the
// pairwise Euclidean distances in float64 on the device, the linkage on the host (ward_linkage.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "common.h"
#include "tri_tiles.h"
#include "ward_linkage.h"

namespace expecto {
namespace {

// A workgroup computes one PD_TILE x PD_TILE tile of the pair matrix (upper triangle, diagonal tiles
// included).  The two panels of PD_TILE points are staged through LDS PD_KS dimensions at a time;
// each of the 256 lanes holds a 4 x 4 micro-tile of pairs and walks the dimensions in order.
constexpr int PD_TILE = 64;
constexpr int PD_KS = 32;
constexpr int PD_LDW = PD_KS + 1;   // LDS row stride in doubles: odd, so 16 points' reads of one k hit 32 banks
constexpr int PD_THREADS = 256;
constexpr long long PD_MAX_N = 1LL << 21;   // the tile count of the upper triangle stays below 2^31

// The tile (bi <= bj) of a workgroup's linear index: pd_tile_of, tri_tiles.h.

// out[pair (i < j)] = sqrt(sum_k (X[i,k] - X[j,k])^2): s = 0, then s = s + t*t for k = 0..d-1 in
// order, the product and the sum rounded separately, the square root correctly rounded -- scipy's
// pdist loop, so the bits are its bits.  Dimensions past d in the last stage are staged as zeros
// for both points: they add +0.0 to a sum that is never -0.0, which leaves it as it is.
__global__ __launch_bounds__(PD_THREADS) void pairwise_euclidean_kernel(const double* __restrict__ X, long long n,
                                                                        long long d, long long ld,
                                                                        double* __restrict__ out, long long T) {
#pragma clang fp contract(off)   // products and sums rounded separately
  __shared__ double As[PD_TILE * PD_LDW];
  __shared__ double Bs[PD_TILE * PD_LDW];
  int bi, bj;
  pd_tile_of(blockIdx.x, T, bi, bj);
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;   // pairs: points i0 + ty + 16 r  x  points j0 + tx + 16 c
  const int lk = tid & 31, lp = tid >> 5;   // loads: dimension lk of points lp + 8 q of both panels
  const long long i0 = (long long)bi * PD_TILE, j0 = (long long)bj * PD_TILE;

  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;

  double ra[8], rb[8];
  auto fetch = [&](long long k0) {
    const long long k = k0 + lk;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long gi = i0 + lp + 8 * q, gj = j0 + lp + 8 * q;
      ra[q] = (k < d && gi < n) ? X[gi * ld + k] : 0.0;
      rb[q] = (k < d && gj < n) ? X[gj * ld + k] : 0.0;
    }
  };
  fetch(0);
  for (long long k0 = 0; k0 < d; k0 += PD_KS) {
    __syncthreads();   // the previous stage has been read
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      As[(lp + 8 * q) * PD_LDW + lk] = ra[q];
      Bs[(lp + 8 * q) * PD_LDW + lk] = rb[q];
    }
    __syncthreads();
    if (k0 + PD_KS < d) fetch(k0 + PD_KS);   // the next stage's loads fly under this stage's arithmetic
#pragma unroll 8
    for (int k = 0; k < PD_KS; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[r] = As[(ty + 16 * r) * PD_LDW + k];
        b[r] = Bs[(tx + 16 * r) * PD_LDW + k];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double t = a[r] - b[c];
          acc[r][c] = acc[r][c] + t * t;
        }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long i = i0 + ty + 16 * r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long long j = j0 + tx + 16 * c;
      if (i < n && j < n && j > i) out[n * i - i * (i + 1) / 2 + (j - i - 1)] = sqrt(acc[r][c]);
    }
  }
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_pairwise_euclidean(const double* X, long long n, long long d, long long ld, double* out, void* stream) {
  EXPECTO_REQUIRE(n >= 0 && d >= 0, "pairwise_euclidean: negative shape");
  EXPECTO_REQUIRE(n <= PD_MAX_N, "pairwise_euclidean: at most 2097152 points per call");
  EXPECTO_REQUIRE(ld >= d, "pairwise_euclidean: row stride ld < d");
  if (n < 2) return EXPECTO_OK;
  EXPECTO_REQUIRE(out && (X || d == 0), "null argument");
  const long long T = (n + PD_TILE - 1) / PD_TILE;
  const long long tiles = T * (T + 1) / 2;
  pairwise_euclidean_kernel<<<dim3((unsigned)tiles), dim3(PD_THREADS), 0, as_stream(stream)>>>(X, n, d, ld, out, T);
  return check_launch("pairwise_euclidean");
}

int expecto_ward_linkage(double* condensed, int n, int* children, double* heights, int* sizes) {
  EXPECTO_REQUIRE(n >= 2, ward_error_text(WARD_ESIZE));
  EXPECTO_REQUIRE(condensed && children && heights && sizes, "null argument");
  const int st = ward_linkage(condensed, n, children, heights, sizes);
  EXPECTO_REQUIRE(st == WARD_OK, ward_error_text(st));
  return EXPECTO_OK;
}

}  // extern "C"
