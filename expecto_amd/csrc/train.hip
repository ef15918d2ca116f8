// Training of ExPecto's expression models (train.py:140-146, train_bootstrap.py:100-106):
// xgboost 0.7 booster='gblinear', objective='reg:linear' with nthread=1 -- cyclic coordinate
// descent on weighted ridge / elastic-net least squares (GBLinear::DoBoost plus the learner's
// round loop; the arithmetic is restated in DESIGN.md "Training gblinear models").
//
//  * gbl_round_kernel        one boosting round of one model per 1024-thread workgroup, with one
//                            set of hyper-parameters for the launch or one per model;
//  * gbl_predict_cols_kernel the gblinear margin on the column-major float32 matrix;
//  * gbl_rmse_kernel         xgboost's weighted rmse.
//
// float32 state, double sums: every float32 product and sum is rounded on its own (no FMA), the
// sums over rows run in double through a fixed tree (lane-sequential, wave butterfly, 16 wave
// partials).  No atomics: a model's result does not depend on the batch around it or on
// scheduling.
#include <hip/hip_runtime.h>

#include "common.h"

#pragma clang fp contract(off)

namespace expecto {

constexpr int kTrainThreads = 1024;                       // 16 waves: 4 per SIMD, <= 128 VGPRs
constexpr int kTrainRows = EXPECTO_GBLINEAR_TRAIN_MAX_ROWS / kTrainThreads;   // rows per lane
constexpr int kTrainWaves = kTrainThreads / 64;
static_assert(kTrainRows * kTrainThreads == EXPECTO_GBLINEAR_TRAIN_MAX_ROWS && kTrainRows % 4 == 0, "row cap");

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// Butterfly sum of a full wave: lane pairs 1 and 2 apart (quad_perm), the two quads of a
// half row (row_half_mirror), the two halves of a row (row_mirror), rows 16 and 32 apart.
// Both partners of a step add the same two numbers, so all 64 lanes end with the same bits.
__device__ __forceinline__ double row_sum(double v) {
  v = v + dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v = v + dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  v = v + dpp_f64<0x141>(v);   // row_half_mirror
  v = v + dpp_f64<0x140>(v);   // row_mirror
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  v = row_sum(v);
  v = v + __shfl_xor(v, 16);
  v = v + __shfl_xor(v, 32);
  return v;
}

// Sum of NV values over the workgroup (every thread calls it; blockDim = 16 waves): wave
// butterflies, the 16 wave partials through `slot` ([NV][16] doubles), one barrier, then lane l
// of every row of 16 lanes takes partial l and the row runs the same butterfly: every thread
// ends with the same bits.  Callers alternate between two slots: a thread can still read the
// slot of call i when another writes call i+1's, and the barrier of call i+1 orders those reads
// before call i+2 reuses it.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* slot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = wave_sum(v[i]);
    if (lane == 0) slot[i * kTrainWaves + wave] = v[i];
  }
  // an LDS-only barrier: __syncthreads() would also wait for every global access in flight, the
  // prefetched column and the store of the last w among them, once per feature.  Nothing a
  // thread writes to global memory here is read by another thread of the launch.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = row_sum(slot[i * kTrainWaves + (lane & 15)]);
}

// xgboost 0.7 CoordinateDelta, in double.
__device__ __forceinline__ double cd_delta(double sg, double sh, double w, double lambda, double alpha) {
  if (sh < 1e-5) return 0.0;
  const double t = w - (sg + lambda * w) / (sh + lambda);
  if (t >= 0.0) return fmax(-(sg + lambda * w + alpha) / (sh + lambda), -w);
  return fmin(-(sg + lambda * w - alpha) / (sh + lambda), -w);
}

// Lane t holds rows k * 1024 + t, k < 24: consecutive lanes read consecutive rows of a column.
// Raw buffer loads over the column's n floats: the hardware range check returns 0 for a row
// past n (no read), so the loads need no per-row test and no per-row address register.  Such a
// slot also has h = 0, y = 0 and g = 0 and adds exact zeros to every sum.
__device__ __forceinline__ void load_col(const float* col, int n, float (&x)[kTrainRows]) {
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(col), 0, n * (int)sizeof(float), 0x00020000);
#pragma unroll
  for (int k = 0; k < kTrainRows; ++k)
    x[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, threadIdx.x * 4, k * kTrainThreads * 4, 0));
}

__device__ __forceinline__ void predict_step(float (&p)[kTrainRows], const float (&x)[kTrainRows], float wj) {
#pragma unroll
  for (int k = 0; k < kTrainRows; ++k)
    p[k] = p[k] + x[k] * wj;
}

struct TrainHyper {
  double eta, lambda, alpha, lambda_bias;
};

// Where a launch's hyper-parameters come from.  One TrainHyper kernel argument serves every model
// of the launch (expecto_gblinear_train_round); a [n_models, 4] table of doubles gives model m its
// own row (expecto_gblinear_train_round_hp).  The row's address depends on blockIdx.x alone and
// nothing is stored before it is read, so the four doubles arrive by scalar loads and stay in
// scalar registers, as the kernel argument does: no lane holds a copy.
__device__ __forceinline__ TrainHyper hyper_of(const TrainHyper& hp, int) { return hp; }
__device__ __forceinline__ TrainHyper hyper_of(const double* hyper, int m) {
  const double* row = hyper + 4 * (long long)m;
  return TrainHyper{row[0], row[1], row[2], row[3]};
}

// One coordinate: sg = sum g*x (sh = sum (h*x)*x in the first round, stored; read afterwards:
// it does not change between rounds), dw from the same numbers on every lane, g += (h*x)*dw.
template <bool FIRST>
__device__ __forceinline__ void cd_step(float (&g)[kTrainRows], const float (&x)[kTrainRows], const float4* hl, int j,
                                        float wj, double shj, float* wm, double* shm, const TrainHyper& hp,
                                        double* slot) {
  constexpr int NV = FIRST ? 2 : 1, SH = NV - 1;   // v[SH] is the sh sum of a first round
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
#pragma unroll
  for (int q = 0; q < kTrainRows / 4; ++q) {
    float4 h4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (FIRST) h4 = hl[q * kTrainThreads + threadIdx.x];
    const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * q + e;
      v[0] = v[0] + (double)(g[k] * x[k]);
      if (FIRST) {
        const float hx = hv[e] * x[k];
        v[SH] = v[SH] + (double)(hx * x[k]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // a quad at a time: hoisting all 24 h loads spills
  }
  block_sum(v, slot);
  if (FIRST) shj = v[SH];
  const float dw = (float)(hp.eta * cd_delta(v[0], shj, (double)wj, hp.lambda, hp.alpha));
  if (threadIdx.x == 0) {
    wm[j] = wj + dw;
    if (FIRST) shm[j] = shj;
  }
#pragma unroll
  for (int q = 0; q < kTrainRows / 4; ++q) {
    const float4 h4 = hl[q * kTrainThreads + threadIdx.x];
    const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * q + e;
      const float hx = hv[e] * x[k];
      g[k] = g[k] + hx * dw;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One round of model m = blockIdx.x.  The lane's 24 gradients stay in registers for the whole
// pass, its 24 row weights in LDS (96 KB, read only by the lane that wrote them), and the
// columns of X come through two register buffers: column j+1 is loaded before column j is
// reduced, so a feature's dependent chain is its reduction, not a memory round trip.
// HP: TrainHyper (by value, for every model) or const double* (a row per model), see hyper_of.
template <bool FIRST, class HP>
__global__ __launch_bounds__(kTrainThreads) void gbl_round_kernel(
    const float* __restrict__ X, long long ld, int n, int F, const float* __restrict__ y, long long y_stride,
    const float* __restrict__ h, long long h_stride, float* w, double* sh, HP hyper, float base_score,
    float* __restrict__ pred) {
  __shared__ float4 hl[kTrainRows / 4 * kTrainThreads];
  __shared__ double slots[2][2 * kTrainWaves];
  const int m = blockIdx.x, t = threadIdx.x;
  const TrainHyper hp = hyper_of(hyper, m);
  float* const wm = w + (long long)m * (F + 1);
  double* const shm = sh + (long long)m * F;
  float b = wm[F];

  // 1. predict: p = (b + base_score) + x_0 w_0 + x_1 w_1 + ... in column order
  float g[kTrainRows], xa[kTrainRows], xb[kTrainRows];
#pragma unroll
  for (int k = 0; k < kTrainRows; ++k) g[k] = b + base_score;
  if (F > 0) load_col(X, n, xa);
#pragma nounroll
  for (int j = 0; j < F; j += 2) {
    const bool more = j + 1 < F;
    if (more) load_col(X + (long long)(j + 1) * ld, n, xb);
    predict_step(g, xa, wm[j]);
    if (!more) break;
    if (j + 2 < F) load_col(X + (long long)(j + 2) * ld, n, xa);
    predict_step(g, xb, wm[j + 1]);
  }
  // the first column of the coordinate pass is on its way during the gradient and bias steps
  if (F > 0) load_col(X, n, xa);

  // 2. gradient g = (p - y) * h; rows past n carry h = 0, x = 0, g = 0
  double v[2] = {0.0, 0.0};
#pragma unroll
  for (int q = 0; q < kTrainRows / 4; ++q) {
    float hv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * q + e;
      const int r = k * kTrainThreads + t;
      float yv = 0.f;
      if (r < n) {
        yv = y[(long long)m * y_stride + r];
        hv[e] = h ? h[(long long)m * h_stride + r] : 1.f;
        if (pred) pred[(long long)m * n + r] = g[k];
      }
      g[k] = (g[k] - yv) * hv[e];
      v[0] = v[0] + (double)g[k];
      v[1] = v[1] + (double)hv[e];
    }
    hl[q * kTrainThreads + t] = make_float4(hv[0], hv[1], hv[2], hv[3]);
  }

  // 3. bias
  int it = 0;
  block_sum(v, slots[it++ & 1]);
  const float db = (float)(hp.eta * (-(v[0] + hp.lambda_bias * (double)b) / (v[1] + hp.lambda_bias)));
  b = b + db;
#pragma unroll
  for (int q = 0; q < kTrainRows / 4; ++q) {
    const float4 h4 = hl[q * kTrainThreads + t];
    const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) g[4 * q + e] = g[4 * q + e] + hv[e] * db;
  }

  // 4. coordinate descent in column order; w_j and sh_j are fetched a step ahead like the column
  float wa = 0.f, wb = 0.f;
  double sa = 0.0, sb = 0.0;
  if (F > 0) {
    wa = wm[0];
    if (!FIRST) sa = shm[0];
  }
#pragma nounroll
  for (int j = 0; j < F; j += 2) {
    const bool more = j + 1 < F;
    if (more) {
      load_col(X + (long long)(j + 1) * ld, n, xb);
      wb = wm[j + 1];
      if (!FIRST) sb = shm[j + 1];
    }
    cd_step<FIRST>(g, xa, hl, j, wa, sa, wm, shm, hp, slots[it++ & 1]);
    if (!more) break;
    if (j + 2 < F) {
      load_col(X + (long long)(j + 2) * ld, n, xa);
      wa = wm[j + 2];
      if (!FIRST) sa = shm[j + 2];
    }
    cd_step<FIRST>(g, xb, hl, j + 1, wb, sb, wm, shm, hp, slots[it++ & 1]);
  }
  if (t == 0) wm[F] = b;
}

// out[m][i] = (b_m + base_score) + sum_j X[j][i] * w_m[j] in column order, float32, product and
// sum rounded separately (gblinear_kernel's rule on the column-major matrix).  One lane per
// row; a chunk's loads go out before its products.
constexpr int kPredChunk = 8;
__global__ __launch_bounds__(256) void gbl_predict_cols_kernel(const float* __restrict__ X, long long ld, int n, int F,
                                                               const float* __restrict__ w, float base_score,
                                                               float* __restrict__ out) {
  const long long m = blockIdx.y;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float* wm = w + m * (F + 1);
  float p = wm[F] + base_score;
  const float* col = X + r;
  for (int j0 = 0; j0 < F; j0 += kPredChunk) {
    float x[kPredChunk];
#pragma unroll
    for (int u = 0; u < kPredChunk; ++u)
      if (j0 + u < F) x[u] = col[(long long)(j0 + u) * ld];
#pragma unroll
    for (int u = 0; u < kPredChunk; ++u)
      if (j0 + u < F) p = p + x[u] * wm[j0 + u];
  }
  out[m * n + r] = p;
}

// xgboost's rmse: sqrt(sum h * (y - p)^2 / sum h), the square and its product with h in
// float32 (EvalRow returns a float, times the float weight), both sums in double.
__global__ __launch_bounds__(kTrainThreads) void gbl_rmse_kernel(const float* __restrict__ pred,
                                                                 const float* __restrict__ y, long long y_stride,
                                                                 const float* __restrict__ h, long long h_stride, int n,
                                                                 double* __restrict__ out) {
  __shared__ double slot[2 * kTrainWaves];
  const long long m = blockIdx.x;
  double v[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += kTrainThreads) {
    const float d = y[m * y_stride + i] - pred[m * n + i];
    const float hv = h ? h[m * h_stride + i] : 1.f;
    const float sq = d * d;
    v[0] = v[0] + (double)(sq * hv);
    v[1] = v[1] + (double)hv;
  }
  block_sum(v, slot);
  if (threadIdx.x == 0) out[m] = sqrt(v[0] / v[1]);
}

// The host side both entry points share: shapes, strides, the row cap, then the launch.
static int check_train_round(const float* X, long long ld, int n, int num_feature, const float* y, long long y_stride,
                             long long h_stride, const float* w, const double* sh) {
  EXPECTO_REQUIRE(n <= EXPECTO_GBLINEAR_TRAIN_MAX_ROWS, "gblinear training holds at most 24576 rows per model");
  EXPECTO_REQUIRE(ld >= n && y_stride >= 0 && h_stride >= 0, "bad stride (ld >= n)");
  EXPECTO_REQUIRE(y && w && (num_feature == 0 || (X && sh)), "null argument");
  return EXPECTO_OK;
}

template <class HP>
static int launch_train_round(const float* X, long long ld, int n, int num_feature, int n_models, const float* y,
                              long long y_stride, const float* h, long long h_stride, float* w, double* sh, int first,
                              HP hyper, float base_score, float* pred, void* stream) {
  const dim3 grid((unsigned)n_models), block(kTrainThreads);
  if (first)
    gbl_round_kernel<true, HP><<<grid, block, 0, as_stream(stream)>>>(X, ld, n, num_feature, y, y_stride, h, h_stride,
                                                                      w, sh, hyper, base_score, pred);
  else
    gbl_round_kernel<false, HP><<<grid, block, 0, as_stream(stream)>>>(X, ld, n, num_feature, y, y_stride, h, h_stride,
                                                                       w, sh, hyper, base_score, pred);
  return check_launch("gblinear_train_round");
}

}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_gblinear_train_round(const float* X, long long ld, int n, int num_feature, int n_models, const float* y,
                                 long long y_stride, const float* h, long long h_stride, float* w, double* sh,
                                 int first, double eta, double lambda, double alpha, double lambda_bias,
                                 float base_score, float* pred, void* stream) {
  EXPECTO_REQUIRE(n >= 0 && num_feature >= 0 && n_models >= 0, "negative shape");
  if (n == 0 || n_models == 0) return EXPECTO_OK;
  if (const int st = check_train_round(X, ld, n, num_feature, y, y_stride, h_stride, w, sh)) return st;
  return launch_train_round(X, ld, n, num_feature, n_models, y, y_stride, h, h_stride, w, sh, first,
                            TrainHyper{eta, lambda, alpha, lambda_bias}, base_score, pred, stream);
}

int expecto_gblinear_train_round_hp(const float* X, long long ld, int n, int num_feature, int n_models, const float* y,
                                    long long y_stride, const float* h, long long h_stride, float* w, double* sh,
                                    int first, const double* hyper, float base_score, float* pred, void* stream) {
  EXPECTO_REQUIRE(n >= 0 && num_feature >= 0 && n_models >= 0, "negative shape");
  if (n == 0 || n_models == 0) return EXPECTO_OK;
  if (const int st = check_train_round(X, ld, n, num_feature, y, y_stride, h_stride, w, sh)) return st;
  EXPECTO_REQUIRE(hyper, "null argument");
  return launch_train_round(X, ld, n, num_feature, n_models, y, y_stride, h, h_stride, w, sh, first, hyper, base_score,
                            pred, stream);
}

int expecto_gblinear_predict_cols(const float* X, long long ld, int n, int num_feature, int n_models, const float* w,
                                  float base_score, float* out, void* stream) {
  EXPECTO_REQUIRE(n >= 0 && num_feature >= 0 && n_models >= 0, "negative shape");
  if (n == 0 || n_models == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(n_models <= 65535, "at most 65535 models per call");
  EXPECTO_REQUIRE(ld >= n, "bad stride (ld >= n)");
  EXPECTO_REQUIRE(w && out && (num_feature == 0 || X), "null argument");
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_models);
  gbl_predict_cols_kernel<<<grid, dim3(256), 0, as_stream(stream)>>>(X, ld, n, num_feature, w, base_score, out);
  return check_launch("gblinear_predict_cols");
}

int expecto_gblinear_rmse(const float* pred, const float* y, long long y_stride, const float* h, long long h_stride,
                          int n, int n_models, double* out, void* stream) {
  EXPECTO_REQUIRE(n >= 0 && n_models >= 0, "negative shape");
  if (n == 0 || n_models == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(y_stride >= 0 && h_stride >= 0, "bad stride");
  EXPECTO_REQUIRE(pred && y && out, "null argument");
  gbl_rmse_kernel<<<dim3((unsigned)n_models), dim3(kTrainThreads), 0, as_stream(stream)>>>(pred, y, y_stride, h,
                                                                                           h_stride, n, out);
  return check_launch("gblinear_rmse");
}

}  // extern "C"
