// Scores of a batch of trained models (train_susztak.py:146-181, train.py:161-184: scipy's pearsonr and
// spearmanr, sklearn's r2_score) and the per-coefficient statistics of a bootstrap batch
// (plot_bootstrapped_coefficients.py:52-76), on the device that trained them.
//
// rank2_kernel: doubled average ranks by counting.  Block (bx, p) owns elements bx*256 .. bx*256+255 of row
// p, one per thread; the whole row streams through LDS in tiles of MT_JTILE values and every thread counts
// the values below and equal to its own.  All lanes read the same LDS address (a broadcast, 16 bytes a
// read), so the loop is two compares and two adds per pair and nothing else.  The last tile is padded with
// NaN, which compares false with everything: the inner loop has no bound check.  A sort would need a
// segmented sort of P rows plus a tie pass and a scatter back; the count is n^2 compares per row but has
// no data-dependent control flow, no atomics and no second pass (DESIGN.md "Model metrics").
//
// model_metrics_kernel: one workgroup of 256 threads per model.
//   Spearman from exact int64 sums of the doubled ranks a (of pred) and b (of y):
//     rho = double(n Sab - Sa Sb) / sqrt(double(n Saa - Sa^2) * double(n Sbb - Sb^2)).
//   A doubled rank is at most 2n, so every term is at most n * n * (2n)^2 = 4 n^4 = 2^62 at n = 32768
//   (the cruder bound n^2 (2n+1)^2 is about 4.6e18): below 2^63.  Integer sums do not depend on their
//   order.
//   Pearson and R2 in float64, two passes (means, then centred sums), pred widened exactly.  Summation
//   order of every float64 sum: thread t adds elements t, t+256, t+512, ... in ascending order onto +0.0;
//   the 256 partials then fold in LDS by p[i] = p[i] + p[i+w] for i < w, w = 128, 64, ..., 1.  Products are
//   rounded before they are added (contraction off).  mean = sum / double(n).
//     pearson = sxy / sqrt(sxx * syy), then clipped to [-1, 1] (a NaN stays);
//     r2 = 1 - ssr / syy, ssr = sum (y - pred)^2; syy == 0: 1.0 if ssr == 0 else 0.0 (sklearn's force_finite).
//   A NaN in the model's pred or y makes all three NaN.
//
// coef_stats_kernel: one thread per coefficient, the B models in ascending order (numpy's order for an
// axis=0 reduction of a C-contiguous array): mean = sum / B, se = sqrt(sum (w - mean)^2 / (B - 1)),
// z = w_main / se, cv = se / |mean|.  Neighbouring threads read neighbouring coefficients.  The deviations
// need the mean, so W is walked twice, as np.std does; the second walk is served by the Infinity Cache
// while W (B * ld * 8 bytes) fits it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"

#pragma clang fp contract(off)

namespace expecto {
namespace {

constexpr int MT_THREADS = 256;              // rank2: elements a block owns; model_metrics: the workgroup
constexpr int MT_JTILE = 2048;               // rank2: values of the row in LDS at a time
constexpr int MT_MAX_ROWS = EXPECTO_METRICS_MAX_ROWS;
constexpr int CS_THREADS = 64;
constexpr int CS_MAX_B = 4096;

template <typename T>
__global__ __launch_bounds__(MT_THREADS) void rank2_kernel(const T* __restrict__ x, long long stride, int n,
                                                           int* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) T tile[MT_JTILE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * MT_THREADS + tid;
  const T* row = x + (long long)blockIdx.y * stride;
  const T nan = (T)__builtin_nan("");
  const T xi = i < n ? row[i] : nan;
  int lt = 0, eq = 0;
  for (int j0 = 0; j0 < n; j0 += MT_JTILE) {
    const int len = n - j0 < MT_JTILE ? n - j0 : MT_JTILE;
    const int len4 = (len + 3) & ~3;
    for (int j = tid; j < len4; j += MT_THREADS) tile[j] = j < len ? row[j0 + j] : nan;
    __syncthreads();
    for (int j = 0; j < len4; j += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const T v = tile[j + u];
        lt += v < xi ? 1 : 0;
        eq += v == xi ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (i < n) out[(long long)blockIdx.y * n + i] = 2 * lt + eq + 1;
}

// v[k] = the sum of the 256 threads' v[k] by the halving tree, in every thread
template <typename T, int NV>
__device__ __forceinline__ void tree_sum(T (&v)[NV], T (*p)[MT_THREADS], int tid) {
#pragma unroll
  for (int k = 0; k < NV; ++k) p[k][tid] = v[k];
  __syncthreads();
  for (int w = MT_THREADS / 2; w >= 1; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < NV; ++k) p[k][tid] = p[k][tid] + p[k][tid + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = p[k][0];
  __syncthreads();
}

__global__ __launch_bounds__(MT_THREADS) void model_metrics_kernel(
    const float* __restrict__ pred, long long pred_stride, const double* __restrict__ y, long long y_stride,
    const int* __restrict__ rank_pred, const int* __restrict__ rank_y, int n, double* __restrict__ out) {
  __shared__ double fsum[4][MT_THREADS];
  __shared__ long long isum[5][MT_THREADS];
  const int tid = threadIdx.x;
  const long long m = blockIdx.x;
  const float* pm = pred + m * pred_stride;
  const double* ym = y + m * y_stride;
  const int* ra = rank_pred + m * n;
  const int* rb = rank_y + (y_stride == 0 ? 0 : m * n);

  double s[2] = {0.0, 0.0};
  long long r[5] = {0, 0, 0, 0, 0};
  int bad = 0;
  for (int i = tid; i < n; i += MT_THREADS) {
    const double p = (double)pm[i], t = ym[i];
    bad |= (p != p) | (t != t);
    s[0] = s[0] + p;
    s[1] = s[1] + t;
    const long long a = ra[i], b = rb[i];
    r[0] += a;
    r[1] += b;
    r[2] += a * b;
    r[3] += a * a;
    r[4] += b * b;
  }
  bad = __syncthreads_or(bad);
  tree_sum(s, fsum, tid);
  tree_sum(r, isum, tid);
  const double mp = s[0] / (double)n, my = s[1] / (double)n;

  double c[4] = {0.0, 0.0, 0.0, 0.0};        // sxy, sxx, syy, ssr
  for (int i = tid; i < n; i += MT_THREADS) {
    const double p = (double)pm[i], t = ym[i];
    const double dx = p - mp, dy = t - my, e = t - p;
    c[0] = c[0] + dx * dy;
    c[1] = c[1] + dx * dx;
    c[2] = c[2] + dy * dy;
    c[3] = c[3] + e * e;
  }
  tree_sum(c, fsum, tid);
  if (tid != 0) return;

  const double nan = __builtin_nan("");
  double pearson = c[0] / sqrt(c[1] * c[2]);
  if (pearson > 1.0) pearson = 1.0;
  if (pearson < -1.0) pearson = -1.0;
  double r2 = 1.0 - c[3] / c[2];
  if (c[2] == 0.0) r2 = c[3] == 0.0 ? 1.0 : 0.0;
  const long long N = n;
  const double num = (double)(N * r[2] - r[0] * r[1]);
  const double da = (double)(N * r[3] - r[0] * r[0]), db = (double)(N * r[4] - r[1] * r[1]);
  const double rho = num / sqrt(da * db);
  out[m * 3 + 0] = bad ? nan : pearson;
  out[m * 3 + 1] = bad ? nan : rho;
  out[m * 3 + 2] = bad ? nan : r2;
}

__global__ __launch_bounds__(CS_THREADS) void coef_stats_kernel(
    const double* __restrict__ W, long long ld, int B, int F, const double* __restrict__ w_main,
    double* __restrict__ mean, double* __restrict__ se, double* __restrict__ z, double* __restrict__ cv) {
  const int f = blockIdx.x * CS_THREADS + threadIdx.x;
  if (f >= F) return;
  const double* col = W + f;
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) s = s + col[(long long)b * ld];
  const double mu = s / (double)B;
  double q = 0.0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) {
    const double d = col[(long long)b * ld] - mu;
    q = q + d * d;
  }
  const double sd = sqrt(q / (double)(B - 1));
  mean[f] = mu;
  se[f] = sd;
  z[f] = w_main[f] / sd;
  cv[f] = sd / fabs(mu);
}

template <typename T>
int rank2(const char* who, const T* x, long long stride, int n, int P, int* out, void* stream) {
  const std::string name(who);
  EXPECTO_REQUIRE(n >= 0 && P >= 0, name + ": negative count");
  EXPECTO_REQUIRE(n <= MT_MAX_ROWS, name + ": at most 32768 values per row");
  EXPECTO_REQUIRE(P <= 65535, name + ": at most 65535 rows per call");
  EXPECTO_REQUIRE(stride >= 0, name + ": negative stride");
  if (n == 0 || P == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(x && out, "null argument");
  rank2_kernel<T><<<dim3((unsigned)((n + MT_THREADS - 1) / MT_THREADS), (unsigned)P), dim3(MT_THREADS), 0,
                    as_stream(stream)>>>(x, stride, n, out);
  return check_launch(who);
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_rank2_f32(const float* x, long long stride, int n, int P, int* out, void* stream) {
  return rank2<float>("rank2_f32", x, stride, n, P, out, stream);
}

int expecto_rank2_f64(const double* x, long long stride, int n, int P, int* out, void* stream) {
  return rank2<double>("rank2_f64", x, stride, n, P, out, stream);
}

int expecto_model_metrics(const float* pred, long long pred_stride, const double* y, long long y_stride,
                          const int* rank_pred, const int* rank_y, int n, int P, double* out, void* stream) {
  EXPECTO_REQUIRE(P >= 0, "model_metrics: negative count");
  EXPECTO_REQUIRE(n >= 2, "model_metrics: at least 2 rows");
  EXPECTO_REQUIRE(n <= MT_MAX_ROWS, "model_metrics: at most 32768 rows");
  EXPECTO_REQUIRE(pred_stride >= 0 && y_stride >= 0, "model_metrics: negative stride");
  if (P == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(pred && y && rank_pred && rank_y && out, "null argument");
  model_metrics_kernel<<<dim3((unsigned)P), dim3(MT_THREADS), 0, as_stream(stream)>>>(pred, pred_stride, y, y_stride,
                                                                                     rank_pred, rank_y, n, out);
  return check_launch("model_metrics");
}

int expecto_bootstrap_coef_stats(const double* W, long long ld, int B, int F, const double* w_main, double* mean,
                                 double* se, double* z, double* cv, void* stream) {
  EXPECTO_REQUIRE(F >= 0, "bootstrap_coef_stats: negative count");
  EXPECTO_REQUIRE(B >= 2 && B <= CS_MAX_B, "bootstrap_coef_stats: 2 <= B <= 4096 models");
  EXPECTO_REQUIRE(ld >= F, "bootstrap_coef_stats: row stride ld < F");
  if (F == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(W && w_main && mean && se && z && cv, "null argument");
  coef_stats_kernel<<<dim3((unsigned)((F + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0, as_stream(stream)>>>(
      W, ld, B, F, w_main, mean, se, z, cv);
  return check_launch("bootstrap_coef_stats");
}

}  // extern "C"
