// Motif similarity clustering (cluster_by_pwm; DESIGN.md "Motif similarity clustering"): the best
// ungapped alignment of every pair of motifs, over all offsets and both strands, on the device; the
// average-linkage tree and its threshold cut on the host (average_linkage.h).
//
// pwm_compare_kernel: one workgroup per MC_TILE x MC_TILE = 16 x 16 tile of motif pairs of the upper
// triangle (tri_tiles.h), one lane per pair, 256 lanes.  The tile's two groups of 16 motifs are staged
// centred (f - 0.25) in LDS, packed by their actual widths; the reverse complement of B is read by
// indexing (column wB-1-j, letter 3-b), never stored.  A lane walks its pair's offsets in ascending
// order and, per offset, sums the D and the R alignment in one pass over the overlap, so the ssa of
// the two strands (the same A columns) is summed once.
//
// Tile size.  LDS per workgroup is 2 groups x (sum of the 16 widths) x 32 B plus 400 B of offsets,
// sized per launch by the widest group of the call: 15 KiB at the 15 columns of a typical motif, so
// the 160 KiB of a CU hold the 8 workgroups (32 waves, 8 per SIMD) that the wave cap admits; 64 KiB
// when every motif has 64 columns, which still leaves 2 workgroups (2 waves per SIMD).  A 32 x 32
// tile would double LDS per workgroup for 4 times the lanes (1024, one workgroup per CU at full
// width) and leave the lanes of a wave further apart in loop count; an 8 x 8 tile is one wave and
// stages twice the columns per pair.  The inner loop is five dependent float64 chains per lane
// (multiply, then add, no contraction), latency-bound within a lane: the 8 waves per SIMD cover it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "average_linkage.h"
#include "common.h"
#include "tri_tiles.h"

#pragma clang fp contract(off)

namespace expecto {
namespace {

constexpr int MC_TILE = 16;
constexpr int MC_THREADS = MC_TILE * MC_TILE;
constexpr int MC_MAX_W = 64;
constexpr long long MC_MAX_M = 4096;
constexpr int MC_META_INTS = 2 * (MC_TILE + 1) + 4 * MC_TILE;   // local column starts, global column starts, widths

__host__ __device__ inline size_t mc_lds_bytes(int group_cols) {
  return (size_t)2 * group_cols * 4 * sizeof(double) + MC_META_INTS * sizeof(int);
}

// Every output of pair (i < j) at scipy's condensed index; A is motif i, B is motif j.
// The second launch bound asks for 8 waves per SIMD: 64 VGPRs, which the kernel fits without scratch.
__global__ __launch_bounds__(MC_THREADS, 8) void pwm_compare_kernel(
    const double* __restrict__ freq, const int* __restrict__ col_ptr, long long M, long long total_cols, int min_w,
    int group_cols, long long T, double* __restrict__ cor, double* __restrict__ ncor, double* __restrict__ dist,
    int* __restrict__ offset, int* __restrict__ strand, int* __restrict__ width) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mc_lds[];
  double* cols = reinterpret_cast<double*>(mc_lds);                   // [2][group_cols][4], centred
  int* l_col = reinterpret_cast<int*>(cols + (size_t)2 * group_cols * 4);   // [2][MC_TILE + 1]
  int* g_col = l_col + 2 * (MC_TILE + 1);                              // [2][MC_TILE]
  int* m_w = g_col + 2 * MC_TILE;                                      // [2][MC_TILE]

  int bi, bj;
  pd_tile_of(blockIdx.x, T, bi, bj);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // widths of the tile's motifs; the device copy of col_ptr is not the one the host checked: a motif
  // that does not fit gets width 0 and its pairs are passed over
  if (tid < 2 * MC_TILE) {
    const int g = tid / MC_TILE, k = tid % MC_TILE;
    const long long m = (long long)(g ? bj : bi) * MC_TILE + k;
    int w = 0, c0 = 0;
    if (m < M) {
      const long long a = col_ptr[m], b = col_ptr[m + 1];
      if (a >= 0 && b - a >= 1 && b - a <= MC_MAX_W && b <= total_cols) {
        w = (int)(b - a);
        c0 = (int)a;
      }
    }
    m_w[tid] = w;
    g_col[tid] = c0;
  }
  __syncthreads();
  if (tid < 2) {
    int at = 0;
    for (int k = 0; k < MC_TILE; ++k) {
      if (at + m_w[tid * MC_TILE + k] > group_cols) m_w[tid * MC_TILE + k] = 0;   // would leave the group's LDS
      l_col[tid * (MC_TILE + 1) + k] = at;
      at += m_w[tid * MC_TILE + k];
    }
    l_col[tid * (MC_TILE + 1) + MC_TILE] = at;
  }
  __syncthreads();
  for (int q = wave; q < 2 * MC_TILE; q += MC_THREADS / 64) {
    const int g = q / MC_TILE, k = q % MC_TILE;
    const int w = m_w[q];
    const double* src = freq + (long long)g_col[q] * 4;
    double* dst = cols + ((size_t)g * group_cols + l_col[g * (MC_TILE + 1) + k]) * 4;
    for (int x = lane; x < 4 * w; x += 64) dst[x] = src[x] - 0.25;
  }
  __syncthreads();

  const int ia = tid / MC_TILE, ib = tid % MC_TILE;
  const long long i = (long long)bi * MC_TILE + ia, j = (long long)bj * MC_TILE + ib;
  const int wA = m_w[ia], wB = m_w[MC_TILE + ib];
  if (i >= M || j >= M || j <= i || wA == 0 || wB == 0) return;
  const double* A = cols + (size_t)l_col[ia] * 4;
  const double* B = cols + ((size_t)group_cols + l_col[(MC_TILE + 1) + ib]) * 4;

  int need = min_w < wA ? min_w : wA;
  need = need < wB ? need : wB;
  double best_ncor = -__builtin_inf(), best_cor = 0.0;
  int best_o = 0, best_s = 0, best_w = 0;
  for (int o = -(wB - need); o <= wA - need; ++o) {
    const int lo = o > 0 ? o : 0, hi = o + wB < wA ? o + wB : wA;
    const int w = hi - lo;
    double ssa = 0.0, num_d = 0.0, ssb_d = 0.0, num_r = 0.0, ssb_r = 0.0;
    for (int c = lo; c < hi; ++c) {
      const double* a = A + 4 * c;
      const double* bd = B + 4 * (c - o);
      const double* br = B + 4 * (wB - 1 - (c - o));
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double av = a[b], dv = bd[b], rv = br[3 - b];
        ssa = ssa + av * av;
        num_d = num_d + av * dv;
        ssb_d = ssb_d + dv * dv;
        num_r = num_r + av * rv;
        ssb_r = ssb_r + rv * rv;
      }
    }
    const double scale_num = (double)w, scale_den = (double)(wA + wB - w);
#pragma unroll
    for (int s = 0; s < 2; ++s) {   // D, then R: at equal Ncor D wins, then the smaller offset
      const double num = s ? num_r : num_d, den2 = ssa * (s ? ssb_r : ssb_d);
      const double c_ = den2 == 0.0 ? 0.0 : num / sqrt(den2);
      const double n_ = c_ * scale_num / scale_den;
      if (n_ > best_ncor || (n_ == best_ncor && s < best_s)) {
        best_ncor = n_;
        best_cor = c_;
        best_o = o;
        best_s = s;
        best_w = w;
      }
    }
  }
  const long long p = M * i - i * (i + 1) / 2 + (j - i - 1);
  const double d = 1.0 - best_ncor;
  cor[p] = best_cor;
  ncor[p] = best_ncor;
  dist[p] = d < 0.0 ? 0.0 : d;
  offset[p] = best_o;
  strand[p] = best_s;
  width[p] = best_w;
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_pwm_compare(const double* freq, const int* col_ptr_host, const int* col_ptr, long long M, int min_w,
                        double* cor, double* ncor, double* dist, int* offset, int* strand, int* width, void* stream) {
  EXPECTO_REQUIRE(M >= 0, "pwm_compare: negative count");
  EXPECTO_REQUIRE(M <= MC_MAX_M, "pwm_compare: " + std::to_string(M) + " motifs; supported are at most 4096");
  EXPECTO_REQUIRE(min_w >= 1, "pwm_compare: min_w must be at least 1");
  if (M == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(col_ptr_host, "null argument");
  EXPECTO_REQUIRE(col_ptr_host[0] == 0, "pwm_compare: col_ptr[0] != 0");
  for (long long m = 0; m < M; ++m) {
    const long long w = (long long)col_ptr_host[m + 1] - col_ptr_host[m];
    EXPECTO_REQUIRE(w >= 0, "pwm_compare: decreasing col_ptr");
    EXPECTO_REQUIRE(w >= 1 && w <= MC_MAX_W,
                    "pwm_compare: motif " + std::to_string(m) + " has width " + std::to_string(w) + "; supported are 1..64");
  }
  if (M < 2) return EXPECTO_OK;   // no pair: nothing is written
  EXPECTO_REQUIRE(freq && col_ptr && cor && ncor && dist && offset && strand && width, "null argument");
  const long long T = (M + MC_TILE - 1) / MC_TILE;
  int group_cols = 0;
  for (long long g = 0; g < T; ++g) {
    const long long end = (g + 1) * MC_TILE < M ? (g + 1) * MC_TILE : M;
    const int c = col_ptr_host[end] - col_ptr_host[g * MC_TILE];
    if (c > group_cols) group_cols = c;
  }
  const size_t lds = mc_lds_bytes(group_cols);
  if (lds > 65536)
    EXPECTO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pwm_compare_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)mc_lds_bytes(MC_TILE * MC_MAX_W)));
  const long long tiles = T * (T + 1) / 2;
  pwm_compare_kernel<<<dim3((unsigned)tiles), dim3(MC_THREADS), lds, as_stream(stream)>>>(
      freq, col_ptr, M, col_ptr_host[M], min_w, group_cols, T, cor, ncor, dist, offset, strand, width);
  return check_launch("pwm_compare");
}

int expecto_average_linkage(double* condensed, int n, int* children, double* heights, int* sizes) {
  EXPECTO_REQUIRE(n >= 2, average_error_text(AVG_ESIZE));
  EXPECTO_REQUIRE(condensed && children && heights && sizes, "null argument");
  const int st = average_linkage(condensed, n, children, heights, sizes);
  EXPECTO_REQUIRE(st == AVG_OK, average_error_text(st));
  return EXPECTO_OK;
}

int expecto_linkage_threshold_cut(const int* children, int n, const double* cor, const double* ncor, double min_cor,
                                  double min_ncor, int* labels, double* mean_cor, double* mean_ncor) {
  EXPECTO_REQUIRE(n >= 2, "threshold cut needs at least 2 points");
  EXPECTO_REQUIRE(children && cor && ncor && labels && mean_cor && mean_ncor, "null argument");
  const int st = linkage_threshold_cut(children, n, cor, ncor, min_cor, min_ncor, labels, mean_cor, mean_ncor);
  EXPECTO_REQUIRE(st == AVG_OK, average_error_text(st));
  return EXPECTO_OK;
}

}  // extern "C"
