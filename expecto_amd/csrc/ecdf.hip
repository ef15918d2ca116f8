// Empirical significance of variant effects against a sorted background (gfx950): per query and
// mark the exact count of background values that are at least as large (expecto_ecdf_tail_counts),
// and the per-variant summaries of -log10 e from a host-made table (expecto_ecdf_summary).
// include/expecto_hip.h states the definitions; ecdf_search.h holds the search arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

#define ECDF_HD __host__ __device__
#include "ecdf_search.h"

namespace expecto {

constexpr int kEcdfK = EXPECTO_ECDF_SPLITTERS;      // splitters per column staged in LDS
constexpr int kEcdfCols = EXPECTO_ECDF_TILE_COLS;   // columns per workgroup: one wave each
constexpr int kEcdfQ = 4;                           // queries per lane, side by side
constexpr int kEcdfVars = 64 * kEcdfQ;              // variants per tile
constexpr int kEcdfThreads = 64 * kEcdfCols;
constexpr int kEcdfLd = kEcdfVars + 1;              // tile row pitch in words (odd: the transposes spread over the banks)
constexpr int kEcdfChunks = 32;                     // workgroups that share a column tile, at most
constexpr size_t kEcdfLds = sizeof(float) * ((size_t)kEcdfCols * kEcdfK + (size_t)kEcdfCols * kEcdfLd);
static_assert(kEcdfLds <= 160 * 1024, "splitters and tile exceed the 160 KiB of LDS");
static_assert(kEcdfThreads <= 1024 && kEcdfVars * kEcdfCols % kEcdfThreads == 0, "tile shape");

// grid: 8 * ceil(col_tiles / 8) * chunks workgroups of 16 waves, in one dimension.  Workgroup L
// belongs to group L % 8 (workgroups of one group share an XCD, and so an L2); group x walks the
// column tiles x, x + 8, ... with `chunks` consecutive workgroups per tile, so the workgroups
// resident on an XCD search the same 16 columns while the variants stream past.  Workgroup
// `chunk` of a tile takes the variant tiles chunk, chunk + chunks, ...
// Per workgroup: wave w stages the splitters of column j0 + w once.  Per variant tile: all
// threads read |x| in runs of 16 marks per variant into the LDS tile [column][variant]; wave w
// searches column w for variants lane, lane + 64, lane + 128, lane + 192 (ecdf_count_ge<4>: the
// pick in LDS, the finish in global memory) and puts the counts back into its tile row; all
// threads store the tile to ge in runs of 16 marks.
__global__ __launch_bounds__(kEcdfThreads) void ecdf_tail_counts_kernel(
    const float* __restrict__ bg, int B, const int* __restrict__ cols, int nc, const float* __restrict__ x,
    long long x_stride, int n, int* __restrict__ ge, EcdfPlan plan, int chunks, int col_tiles) {
  extern __shared__ __attribute__((aligned(16))) float ecdf_lds[];
  float* const tile = ecdf_lds + (size_t)kEcdfCols * kEcdfK;
  const int L = blockIdx.x;
  const int q = L >> 3;
  const int ct = (q / chunks) * 8 + (L & 7);
  const int chunk = q % chunks;
  if (ct >= col_tiles) return;   // the whole workgroup
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int j0 = ct * kEcdfCols;
  const bool has_col = j0 + w < nc;
  const float* const col = bg + (long long)cols[has_col ? j0 + w : j0] * B;
  float* const spl = ecdf_lds + (size_t)w * kEcdfK;
  if (has_col)
    for (int i = lane; i < plan.m; i += 64) spl[i] = col[ecdf_splitter_pos(plan, i)];
  // the load / store phases: thread t moves mark jj of variants t / 16 + 64 i
  const int jj = t % kEcdfCols;
  const bool io_col = j0 + jj < nc;
  const long long xc = io_col ? cols[j0 + jj] : 0;
  const int vtiles = (n + kEcdfVars - 1) / kEcdfVars;
  for (int vt = chunk; vt < vtiles; vt += chunks) {
    const long long v0 = (long long)vt * kEcdfVars;
    __syncthreads();   // the splitters; every thread is done with the previous tile
    if (io_col) {
#pragma unroll
      for (int i = 0; i < kEcdfVars * kEcdfCols / kEcdfThreads; ++i) {
        const int vl = (t + kEcdfThreads * i) / kEcdfCols;
        const long long v = v0 + vl;
        tile[jj * kEcdfLd + vl] = v < n ? fabsf(x[v * x_stride + xc]) : 0.0f;
      }
    }
    __syncthreads();
    if (has_col) {
      float a[kEcdfQ];
      int g[kEcdfQ];
#pragma unroll
      for (int k = 0; k < kEcdfQ; ++k) a[k] = tile[w * kEcdfLd + lane + 64 * k];
      ecdf_count_ge<kEcdfQ>(col, B, plan, spl, a, g);
#pragma unroll
      for (int k = 0; k < kEcdfQ; ++k) tile[w * kEcdfLd + lane + 64 * k] = __int_as_float(g[k]);
    }
    __syncthreads();
    if (io_col) {
#pragma unroll
      for (int i = 0; i < kEcdfVars * kEcdfCols / kEcdfThreads; ++i) {
        const int vl = (t + kEcdfThreads * i) / kEcdfCols;
        const long long v = v0 + vl;
        if (v < n) ge[v * nc + j0 + jj] = __float_as_int(tile[jj * kEcdfLd + vl]);
      }
    }
  }
}

// One wave per variant.  Lane l takes marks l, l + 64, ...: the -log10 e terms from the table summed
// from -0.0 in that order, then folded p[l] += p[l + s], s = 32 .. 1 (S of expecto_variant_contrib);
// the maximum, the lowest mark of the smallest count and the number of counts below k_alpha fold
// the same way.
__global__ __launch_bounds__(64) void ecdf_summary_kernel(const int* __restrict__ ge, int nc,
                                                          const double* __restrict__ lut, int k_alpha,
                                                          double* __restrict__ mean_nlog,
                                                          double* __restrict__ max_nlog, int* __restrict__ top,
                                                          int* __restrict__ n_sig) {
#pragma clang fp contract(off)
  const long long v = blockIdx.x;
  const int lane = threadIdx.x;
  double acc = -0.0, mx = -INFINITY;
  long long best = 0x7fffffffffffffffLL;   // (count << 32) | mark
  int sig = 0, bad = 0;
  for (int j = lane; j < nc; j += 64) {
    const int g = ge[v * nc + j];
    const bool ok = g >= 0;
    const double term = lut[ok ? g : 0];
    acc += term;
    mx = fmax(mx, term);
    const long long key = ((long long)(ok ? g : 0) << 32) | (long long)j;
    best = ok && key < best ? key : best;
    sig += ok && g < k_alpha ? 1 : 0;
    bad |= ok ? 0 : 1;
  }
  for (int s = 32; s > 0; s >>= 1) {
    acc += __shfl_down(acc, s, 64);
    mx = fmax(mx, __shfl_down(mx, s, 64));
    const long long other = __shfl_down(best, s, 64);
    best = other < best ? other : best;
    sig += __shfl_down(sig, s, 64);
    bad |= __shfl_down(bad, s, 64);
  }
  if (lane == 0) {
    const double nan64 = __builtin_nan("");
    mean_nlog[v] = bad ? nan64 : acc / (double)nc;
    max_nlog[v] = bad ? nan64 : mx;
    top[v] = bad ? -1 : (int)(best & 0xffffffffLL);
    n_sig[v] = bad ? -1 : sig;
  }
}

}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_ecdf_tail_counts(const float* bg, int B, int C, const int* cols_host, const int* cols, int nc,
                             const float* x, long long x_stride, int n, int* ge, void* stream) {
  EXPECTO_REQUIRE(B >= 1 && B <= 2147483646, "bad background length (1 <= B <= 2^31 - 2)");
  EXPECTO_REQUIRE(C >= 1 && nc >= 1 && nc <= C && n >= 0, "bad shape (1 <= nc <= C, n >= 0)");
  EXPECTO_REQUIRE(cols_host, "null argument");
  for (int j = 0; j < nc; ++j)
    EXPECTO_REQUIRE(cols_host[j] >= 0 && cols_host[j] < C && (j == 0 || cols_host[j] > cols_host[j - 1]),
                    "cols must be ascending mark indices in 0..C-1");
  EXPECTO_REQUIRE(x_stride >= (long long)cols_host[nc - 1] + 1, "x_stride below max(cols) + 1");
  if (n == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(bg && cols && x && ge, "null argument");
  const EcdfPlan plan = ecdf_plan(B, kEcdfK);
  const int col_tiles = (nc + kEcdfCols - 1) / kEcdfCols;
  const int vtiles = (n + kEcdfVars - 1) / kEcdfVars;
  const int chunks = vtiles < kEcdfChunks ? vtiles : kEcdfChunks;
  EXPECTO_REQUIRE((long long)((col_tiles + 7) / 8) * 8 * chunks <= 2147483647LL, "too many marks");
  EXPECTO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ecdf_tail_counts_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEcdfLds));
  const dim3 grid((col_tiles + 7) / 8 * 8 * chunks);
  ecdf_tail_counts_kernel<<<grid, dim3(kEcdfThreads), kEcdfLds, as_stream(stream)>>>(bg, B, cols, nc, x, x_stride, n,
                                                                                     ge, plan, chunks, col_tiles);
  return check_launch("ecdf_tail_counts");
}

int expecto_ecdf_summary(const int* ge, int n, int nc, const double* lut, int B, int k_alpha, double* mean_nlog,
                         double* max_nlog, int* top, int* n_sig, void* stream) {
  EXPECTO_REQUIRE(B >= 1 && B <= 2147483646, "bad background length (1 <= B <= 2^31 - 2)");
  EXPECTO_REQUIRE(nc >= 1 && n >= 0, "bad shape (nc >= 1, n >= 0)");
  EXPECTO_REQUIRE(k_alpha >= 0 && k_alpha <= B + 1, "k_alpha outside 0..B+1");
  if (n == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(ge && lut && mean_nlog && max_nlog && top && n_sig, "null argument");
  ecdf_summary_kernel<<<dim3(n), dim3(64), 0, as_stream(stream)>>>(ge, nc, lut, k_alpha, mean_nlog, max_nlog, top,
                                                                   n_sig);
  return check_launch("ecdf_summary");
}

}  // extern "C"
