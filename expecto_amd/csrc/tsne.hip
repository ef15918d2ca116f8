// Exact t-SNE of one small matrix (cluster_and_viz.py:60-66: TSNE(n_components=2).fit_transform(X)):
// sklearn's _joint_probabilities over _binary_search_perplexity, and its _gradient_descent over
// _kl_divergence with one degree of freedom.  The arithmetic is the fixed one include/expecto_hip.h
// states: float64, products and sums rounded separately, every sum over a row or over the rows in
// wave order, no atomics.  One wave owns one row, whatever the block size, so the bits do not depend
// on the launch geometry.  Iterations are separated by kernel boundaries: pass A (the row sums of
// num), pass B (Z from those, the gradient row, the update), and one closing launch per call.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>

#include "common.h"

#pragma clang fp contract(off)

namespace expecto {
namespace {

constexpr int TS_MAX_N = 4096;
constexpr int TS_MAX_D = 128;
constexpr int TS_WAVE = 64;
constexpr int TS_ROWS = 4;                 // rows (waves) per workgroup of the row kernels
constexpr int TS_MAX_STEPS = 100;          // _binary_search_perplexity: n_steps
constexpr double TS_TOL = 1e-5;            //                            PERPLEXITY_TOLERANCE
constexpr double TS_TINY_SUM = 1e-8;       //                            EPSILON_DBL
constexpr double TS_EPS = DBL_EPSILON;     // _t_sne.py: MACHINE_EPSILON

// workspace, in doubles: the second copy of Y [2n], z [n], g [2n], the rows' error sums [n];
// the affinities use [0, n] of it (the rows' sums and T)
constexpr long long tsne_workspace_doubles(long long n) { return 6 * n; }

__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }

// Steps 2 and 3 of the wave order: every lane brings its own chain's sum, all lanes receive s_0.
__device__ __forceinline__ double wave_fold(double s) {
#pragma unroll
  for (int w = TS_WAVE / 2; w > 0; w >>= 1) s = s + __shfl_down(s, w, TS_WAVE);
  return __shfl(s, 0, TS_WAVE);
}

// The wave-order sum of a[0..m) by one whole wave.
__device__ __forceinline__ double wave_sum(const double* __restrict__ a, int m, int lane) {
  double s = 0.0;
  for (int j = lane; j < m; j += TS_WAVE) s = s + a[j];
  return wave_fold(s);
}

// ---- affinities ------------------------------------------------------------------------------

// One wave per row: the row's squared distances into LDS, the bisection on beta, and the row of
// conditional probabilities into C (the caller's P, symmetrised in place afterwards).
__global__ __launch_bounds__(TS_WAVE) void tsne_conditional_kernel(const double* __restrict__ X, int n, int d,
                                                                   long long ld, double log_perplexity,
                                                                   double* __restrict__ C, double* __restrict__ beta_out,
                                                                   int* __restrict__ steps_out) {
  __shared__ double D[TS_MAX_N];
  __shared__ double xi[TS_MAX_D];
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  if (i >= n) return;
  for (int t = lane; t < d; t += TS_WAVE) xi[t] = X[(long long)i * ld + t];
  __syncthreads();
  for (int j = lane; j < n; j += TS_WAVE) {
    const double* xj = X + (long long)j * ld;
    double s = 0.0;
    for (int t = 0; t < d; ++t) {
      const double u = xi[t] - xj[t];
      s = s + u * u;
    }
    D[j] = s;
  }
  __syncthreads();

  const double inf = __builtin_inf();
  double beta = 1.0, beta_min = -inf, beta_max = inf;
  double used = 1.0, S = 1.0;
  int steps = 0;
  for (int step = 0; step < TS_MAX_STEPS; ++step) {
    double s = 0.0;
    for (int j = lane; j < n; j += TS_WAVE)
      if (j != i) s = s + exp(-D[j] * beta);
    S = wave_fold(s);
    if (S == 0.0) S = TS_TINY_SUM;
    double e = 0.0;
    for (int j = lane; j < n; j += TS_WAVE)
      if (j != i) {
        const double p = exp(-D[j] * beta) / S;
        e = e + D[j] * p;
      }
    const double H = log(S) + beta * wave_fold(e);
    const double diff = H - log_perplexity;
    used = beta;
    steps = step + 1;
    if (fabs(diff) <= TS_TOL) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == inf ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -inf ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
  double* row = C + (long long)i * n;
  for (int j = lane; j < n; j += TS_WAVE) row[j] = j == i ? 0.0 : exp(-D[j] * used) / S;
  if (lane == 0) {
    beta_out[i] = used;
    steps_out[i] = steps;
  }
}

// r[i] = the wave-order sum over j of (c_ij + c_ji).
__global__ __launch_bounds__(TS_ROWS * TS_WAVE) void tsne_joint_rows_kernel(const double* __restrict__ C, int n,
                                                                            double* __restrict__ r) {
  const int lane = threadIdx.x % TS_WAVE;
  const int i = blockIdx.x * TS_ROWS + threadIdx.x / TS_WAVE;
  if (i >= n) return;
  double s = 0.0;
  for (int j = lane; j < n; j += TS_WAVE)
    if (j != i) s = s + (C[(long long)i * n + j] + C[(long long)j * n + i]);
  s = wave_fold(s);
  if (lane == 0) r[i] = s;
}

__global__ __launch_bounds__(TS_WAVE) void tsne_joint_total_kernel(const double* __restrict__ r, int n,
                                                                   double* __restrict__ T) {
  const double s = wave_sum(r, n, threadIdx.x);
  if (threadIdx.x == 0) *T = s;
}

// P_ij = P_ji from c_ij and c_ji, in place: the lane of (i, j), i < j, reads both and writes both.
__global__ __launch_bounds__(256) void tsne_joint_kernel(double* __restrict__ P, int n, const double* __restrict__ T) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)n * n) return;
  const int i = (int)(e / n), j = (int)(e % n);
  if (i == j) {
    P[e] = 0.0;
  } else if (i < j) {
    const long long f = (long long)j * n + i;
    const double v = dmax((P[e] + P[f]) / dmax(*T, TS_EPS), TS_EPS);
    P[e] = v;
    P[f] = v;
  }
}

// ---- descent ---------------------------------------------------------------------------------

// Pass A: z[i] = the wave-order sum over j of num_ij.
__global__ __launch_bounds__(TS_ROWS * TS_WAVE) void tsne_pass_a_kernel(const double* __restrict__ Y, int n,
                                                                        double* __restrict__ z) {
  const int lane = threadIdx.x % TS_WAVE;
  const int i = blockIdx.x * TS_ROWS + threadIdx.x / TS_WAVE;
  if (i >= n) return;
  const double y0 = Y[2 * i], y1 = Y[2 * i + 1];
  double s = 0.0;
  for (int j = lane; j < n; j += TS_WAVE) {
    if (j == i) continue;
    const double a = y0 - Y[2 * j], b = y1 - Y[2 * j + 1];
    s = s + 1.0 / (1.0 + (a * a + b * b));
  }
  s = wave_fold(s);
  if (lane == 0) z[i] = s;
}

// Pass B: Z from z (once per workgroup), the row's gradient, and the row's update: Y_in is only
// read, Y_out only written.  On the call's last iteration the gradient entries (after the gain) go
// to g, and with ERR the row's share of the error to err.
template <bool ERR>
__global__ __launch_bounds__(TS_ROWS * TS_WAVE) void tsne_pass_b_kernel(
    const double* __restrict__ P, int n, double exaggeration, const double* __restrict__ Y_in,
    double* __restrict__ Y_out, double* __restrict__ update, double* __restrict__ gains, double momentum,
    double learning_rate, const double* __restrict__ z, double* __restrict__ g_out, double* __restrict__ err,
    int last) {
  __shared__ double Z_s;
  const int lane = threadIdx.x % TS_WAVE;
  const int i = blockIdx.x * TS_ROWS + threadIdx.x / TS_WAVE;
  if (threadIdx.x < TS_WAVE) {
    const double s = wave_sum(z, n, lane);
    if (lane == 0) Z_s = s;
  }
  __syncthreads();
  if (i >= n) return;
  const double Z = Z_s;
  const double y0 = Y_in[2 * i], y1 = Y_in[2 * i + 1];
  const double* p = P + (long long)i * n;
  double g0 = 0.0, g1 = 0.0, e = 0.0;
  for (int j = lane; j < n; j += TS_WAVE) {
    if (j == i) continue;
    const double a = y0 - Y_in[2 * j], b = y1 - Y_in[2 * j + 1];
    const double num = 1.0 / (1.0 + (a * a + b * b));
    const double q = dmax(num / Z, TS_EPS);
    const double pe = exaggeration * p[j];
    const double t = (pe - q) * num;
    g0 = g0 + t * a;
    g1 = g1 + t * b;
    if (ERR) e = e + pe * log(dmax(pe, TS_EPS) / q);
  }
  g0 = wave_fold(g0);
  g1 = wave_fold(g1);
  if (ERR) e = wave_fold(e);
  if (lane < 2) {
    const int c = 2 * i + lane;
    double g = 4.0 * (lane == 0 ? g0 : g1);
    const double u = update[c];
    double gain = gains[c];
    gain = u * g < 0.0 ? gain + 0.2 : gain * 0.8;
    gain = dmax(gain, 0.01);
    g = g * gain;
    const double un = momentum * u - learning_rate * g;
    gains[c] = gain;
    update[c] = un;
    Y_out[c] = (lane == 0 ? y0 : y1) + un;
    if (last) g_out[c] = g;
  }
  if (ERR && lane == 0) err[i] = e;
}

// The call's closing launch: the statistics of the last iteration, and Y back into the caller's
// buffer when the iterations ended in the workspace's copy.
__global__ __launch_bounds__(TS_WAVE) void tsne_close_kernel(int n, const double* __restrict__ g,
                                                             const double* __restrict__ z, const double* __restrict__ err,
                                                             int want_error, double* __restrict__ stats,
                                                             const double* __restrict__ Y_from, double* __restrict__ Y_to) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int j = lane; j < 2 * n; j += TS_WAVE) s = s + g[j] * g[j];
  s = wave_fold(s);
  const double Z = wave_sum(z, n, lane);
  double E = 0.0;
  if (want_error) E = wave_sum(err, n, lane);
  if (lane == 0) {
    if (want_error) stats[0] = E;
    stats[1] = sqrt(s);
    stats[2] = Z;
  }
  if (Y_from)
    for (int j = lane; j < 2 * n; j += TS_WAVE) Y_to[j] = Y_from[j];
}

const char* tsne_check_n(long long n) { return n < 2 || n > TS_MAX_N ? "tsne: n must lie in [2, 4096]" : nullptr; }

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

size_t expecto_tsne_workspace(long long n) {
  return tsne_check_n(n) ? 0 : (size_t)(8 * tsne_workspace_doubles(n));
}

int expecto_tsne_affinities(const double* X, long long n, long long d, long long ld, double perplexity, double* P,
                            double* beta, int* steps, void* workspace, size_t workspace_bytes, void* stream) {
  if (const char* err = tsne_check_n(n)) EXPECTO_REQUIRE(false, err);
  EXPECTO_REQUIRE(d >= 1 && d <= TS_MAX_D, "tsne: d must lie in [1, 128]");
  EXPECTO_REQUIRE(ld >= d, "tsne: row stride ld < d");
  EXPECTO_REQUIRE(perplexity > 0.0 && perplexity < (double)n, "tsne: perplexity must lie in (0, n)");
  EXPECTO_REQUIRE(X && P && beta && steps && workspace, "null argument");
  EXPECTO_REQUIRE(workspace_bytes >= expecto_tsne_workspace(n), "tsne_affinities: workspace too small (expecto_tsne_workspace)");
  EXPECTO_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "tsne_affinities: workspace not 8-byte aligned");
  hipStream_t s = as_stream(stream);
  double* r = static_cast<double*>(workspace);
  double* T = r + n;
  const unsigned row_blocks = (unsigned)((n + TS_ROWS - 1) / TS_ROWS);
  tsne_conditional_kernel<<<dim3((unsigned)n), dim3(TS_WAVE), 0, s>>>(X, (int)n, (int)d, ld, std::log(perplexity), P,
                                                                       beta, steps);
  tsne_joint_rows_kernel<<<dim3(row_blocks), dim3(TS_ROWS * TS_WAVE), 0, s>>>(P, (int)n, r);
  tsne_joint_total_kernel<<<dim3(1), dim3(TS_WAVE), 0, s>>>(r, (int)n, T);
  tsne_joint_kernel<<<dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, s>>>(P, (int)n, T);
  return check_launch("tsne_affinities");
}

int expecto_tsne_descend(const double* P, long long n, double exaggeration, double* Y, double* update, double* gains,
                         double momentum, double learning_rate, long long n_iter, int want_error, double* stats,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (const char* err = tsne_check_n(n)) EXPECTO_REQUIRE(false, err);
  EXPECTO_REQUIRE(n_iter >= 0 && n_iter <= 0x7fffffffLL, "tsne_descend: n_iter must lie in [0, 2^31)");
  EXPECTO_REQUIRE(std::isfinite(exaggeration) && std::isfinite(momentum) && std::isfinite(learning_rate),
                  "tsne_descend: exaggeration, momentum and learning_rate must be finite");
  EXPECTO_REQUIRE(P && Y && update && gains && stats && workspace, "null argument");
  EXPECTO_REQUIRE(workspace_bytes >= expecto_tsne_workspace(n), "tsne_descend: workspace too small (expecto_tsne_workspace)");
  EXPECTO_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "tsne_descend: workspace not 8-byte aligned");
  if (n_iter == 0) return EXPECTO_OK;
  hipStream_t s = as_stream(stream);
  double* Y2 = static_cast<double*>(workspace);
  double* z = Y2 + 2 * n;
  double* g = z + n;
  double* err = g + 2 * n;
  const dim3 grid((unsigned)((n + TS_ROWS - 1) / TS_ROWS)), block(TS_ROWS * TS_WAVE);
  for (long long it = 0; it < n_iter; ++it) {
    const double* in = it % 2 ? Y2 : Y;
    double* out = it % 2 ? Y : Y2;
    const int last = it == n_iter - 1;
    tsne_pass_a_kernel<<<grid, block, 0, s>>>(in, (int)n, z);
    if (last && want_error)
      tsne_pass_b_kernel<true><<<grid, block, 0, s>>>(P, (int)n, exaggeration, in, out, update, gains, momentum,
                                                      learning_rate, z, g, err, 1);
    else
      tsne_pass_b_kernel<false><<<grid, block, 0, s>>>(P, (int)n, exaggeration, in, out, update, gains, momentum,
                                                       learning_rate, z, g, err, last);
  }
  tsne_close_kernel<<<dim3(1), dim3(TS_WAVE), 0, s>>>((int)n, g, z, err, want_error, stats, n_iter % 2 ? Y2 : nullptr, Y);
  return check_launch("tsne_descend");
}

}  // extern "C"
