// In-silico saturation mutagenesis (gfx950): every SNV of a region enumerated from the device
// genome, and the expression scoring of their chromatin rows for M gblinear models fused with the
// fwd/rc average and the exp-decay placement, so that the [n, 10*nfeat] float64 feature matrices
// of the unfused chain (expecto_fwd_rc_average -> expecto_variant_reduce_lut ->
// expecto_gblinear_predict per model) never exist.  Bitwise the chain's results.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

namespace expecto {

// Slot 3p + j of position p: the j-th base code (0=A 1=G 2=C 3=T) that is not the genome's.
__global__ void ism_variants_kernel(const uint8_t* __restrict__ genome, long long start, int L,
                                    long long* __restrict__ var_off, uint8_t* __restrict__ ref_code,
                                    uint8_t* __restrict__ alt_code, uint8_t* __restrict__ valid) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= L) return;
  const long long g = start + p;
  const unsigned c = genome[g];
  const bool base = c < 4u;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const long long s = 3LL * p + j;
    var_off[s] = g;
    ref_code[s] = (uint8_t)c;
    alt_code[s] = (uint8_t)(base ? (unsigned)j + ((unsigned)j >= c ? 1u : 0u) : c);
    valid[s] = base ? 1 : 0;
  }
}

constexpr int kIsmThreads = 256;   // one thread per model in the scoring phase: 218 tissue models fit one workgroup

// The [n_shift][10] exp-decay weights of slot v (variant_reduce_kernel's prologue; strand_plus is
// the gene's, one per call).
__device__ __forceinline__ void ism_weights_lds(long long dist_v, int strand_plus, const int* __restrict__ shifts,
                                                int n_shift, const double* __restrict__ lut, int lut_len,
                                                double* wsh) {
  const double decay[5] = {0.01, 0.02, 0.05, 0.1, 0.2};
  for (int j = threadIdx.x; j < n_shift; j += blockDim.x) {
    const long long sgn = strand_plus ? 1 : -1;
    const long long d = dist_v * sgn + (long long)shifts[j] * sgn;
    const double fl = floor(fabs((double)d) / 200.0);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      // host table when it covers the distance, else the device exp (never a read past the table)
      const double e = lut && fl < (double)lut_len ? lut[k * lut_len + (long long)fl] : exp(-decay[k] * fl);
      wsh[j * 10 + k] = d <= 0 ? e : 0.0;
      wsh[j * 10 + 5 + k] = d >= 0 ? e : 0.0;
    }
  }
}

// float32(feature) of decay row k, mark column col, of the chromatin rows y[(s*strand_stride + j*n + v)]:
// (fwd + rc) / 2 in float32 (fwd_rc_avg_kernel), the shifts summed in float64 from -0.0 in their
// order (variant_reduce_kernel), the DMatrix rounding of gblinear_kernel.
__device__ __forceinline__ float ism_feature(const float* __restrict__ y, long long strand_stride, int n_shift, int n,
                                             long long v, int nfeat, int col, const double* wsh, int k) {
#pragma clang fp contract(off)
  double acc = -0.0;
  for (int j = 0; j < n_shift; ++j) {
    const long long o = ((long long)j * n + v) * nfeat + col;
    const float e = (y[o] + y[o + strand_stride * nfeat]) / 2.0f;
    acc += (double)e * wsh[j * 10 + k];
  }
  return (float)acc;
}

// grid: (n / 3 positions, ceil(M / 256) model blocks); 256 threads.  Dynamic LDS: the [n_shift][10]
// f64 weights of the position's three slots, then the current decay row of the four alleles'
// features as float4 [nk] (ref, alt 0, alt 1, alt 2).  Per decay row k = 0..9: every thread builds
// its marks' four features, then thread m walks the nk columns k*nk + f in order with one weight
// load and one 16-byte LDS broadcast read per column feeding four independent float32 chains
// (psum = psum + x * w, every product and sum rounded on its own).  The ref row is built and
// scored once per position; each model's weights are read once per position.
__global__ __launch_bounds__(kIsmThreads) void ism_score_kernel(
    const float* __restrict__ y_ref, const float* __restrict__ y_alt, long long strand_stride,
    const long long* __restrict__ dist, int strand_plus, const int* __restrict__ shifts, int n_shift, int n, int nfeat,
    const double* __restrict__ lut, int lut_len, const int* __restrict__ keep, int nk, const float* __restrict__ w,
    const float* __restrict__ init, int M, const uint8_t* __restrict__ valid, float* __restrict__ alt_pred,
    float* __restrict__ ref_pred, double* __restrict__ sed) {
#pragma clang fp contract(off)   // products rounded before the sum, as the chain's kernels
  extern __shared__ __attribute__((aligned(16))) double ism_lds[];
  double* const wsh = ism_lds;                                                    // [3][n_shift][10]
  float4* const rows = reinterpret_cast<float4*>(ism_lds + 30 * (size_t)n_shift);  // [nk]
  const long long p = blockIdx.x, v0 = 3 * p;
  const int t = threadIdx.x;
  const int m = blockIdx.y * kIsmThreads + t;
  const long long n_pos = n / 3;
  const bool ok0 = valid[v0] != 0, ok1 = valid[v0 + 1] != 0, ok2 = valid[v0 + 2] != 0;
  const float nanf32 = __builtin_nanf("");
  const double nanf64 = __builtin_nan("");
  if (!(ok0 || ok1 || ok2)) {   // the whole workgroup: a position that is not a base
    if (m < M) {
      ref_pred[m * n_pos + p] = nanf32;
      for (int r = 0; r < 3; ++r) {
        alt_pred[(long long)m * n + v0 + r] = nanf32;
        sed[(long long)m * n + v0 + r] = nanf64;
      }
    }
    return;
  }
  for (int r = 0; r < 3; ++r)
    ism_weights_lds(dist[v0 + r], strand_plus, shifts, n_shift, lut, lut_len, wsh + 10 * (size_t)n_shift * r);
  float ps0 = 0.f, ps1 = 0.f, ps2 = 0.f, ps3 = 0.f;
  if (m < M) ps0 = ps1 = ps2 = ps3 = init[m];
  for (int k = 0; k < 10; ++k) {
    __syncthreads();   // the weights (k = 0); every thread is done with the previous decay row
    for (int f = t; f < nk; f += kIsmThreads) {
      const int col = keep[f];
      float4 x;
      x.x = ism_feature(y_ref, strand_stride, n_shift, n, v0, nfeat, col, wsh, k);
      x.y = ism_feature(y_alt, strand_stride, n_shift, n, v0, nfeat, col, wsh, k);
      x.z = ism_feature(y_alt, strand_stride, n_shift, n, v0 + 1, nfeat, col, wsh + 10 * (size_t)n_shift, k);
      x.w = ism_feature(y_alt, strand_stride, n_shift, n, v0 + 2, nfeat, col, wsh + 20 * (size_t)n_shift, k);
      rows[f] = x;
    }
    __syncthreads();
    if (m < M) {
      const float* wk = w + (long long)k * nk * M + m;
#pragma unroll 8
      for (int f = 0; f < nk; ++f) {
        const float wv = wk[(long long)f * M];
        const float4 x = rows[f];
        ps0 = ps0 + x.x * wv;
        ps1 = ps1 + x.y * wv;
        ps2 = ps2 + x.z * wv;
        ps3 = ps3 + x.w * wv;
      }
    }
  }
  if (m >= M) return;
  ref_pred[m * n_pos + p] = ps0;
  const long long o = (long long)m * n + v0;
  alt_pred[o] = ok0 ? ps1 : nanf32;
  alt_pred[o + 1] = ok1 ? ps2 : nanf32;
  alt_pred[o + 2] = ok2 ? ps3 : nanf32;
  sed[o] = ok0 ? (double)ps1 - (double)ps0 : nanf64;
  sed[o + 1] = ok1 ? (double)ps2 - (double)ps0 : nanf64;
  sed[o + 2] = ok2 ? (double)ps3 - (double)ps0 : nanf64;
}

// One wave per model: S(|sed|) and S(sed) over the n slots, S as expecto_variant_contrib defines it
// (lane l adds terms l, l + 64, ... from -0.0, then p[l] += p[l + s] for s = 32 .. 1); an invalid
// slot's term is -0.0, which changes no sum.
__global__ __launch_bounds__(64) void ism_summary_kernel(const double* __restrict__ sed,
                                                         const uint8_t* __restrict__ valid, int n,
                                                         double* __restrict__ potential,
                                                         double* __restrict__ direction) {
#pragma clang fp contract(off)
  const long long m = blockIdx.x;
  const int lane = threadIdx.x;
  double a = -0.0, d = -0.0;
  for (int i = lane; i < n; i += 64) {
    const bool ok = valid[i] != 0;
    const double x = sed[m * n + i];
    a += ok ? fabs(x) : -0.0;
    d += ok ? x : -0.0;
  }
  for (int s = 32; s > 0; s >>= 1) {
    a += __shfl_down(a, s, 64);
    d += __shfl_down(d, s, 64);
  }
  if (lane == 0) {
    potential[m] = n > 0 ? a : 0.0;
    direction[m] = n > 0 ? d : 0.0;
  }
}

}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_ism_variants(const uint8_t* genome, long long genome_len, long long start, int L, long long* var_off,
                         uint8_t* ref_code, uint8_t* alt_code, uint8_t* valid, void* stream) {
  EXPECTO_REQUIRE(L >= 0 && L <= (1 << 30) / 3, "bad region length");
  EXPECTO_REQUIRE(start >= 0 && genome_len >= 0 && start <= genome_len - L, "region outside the genome");
  if (L == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(genome && var_off && ref_code && alt_code && valid, "null argument");
  ism_variants_kernel<<<dim3((L + 255) / 256), dim3(256), 0, as_stream(stream)>>>(genome, start, L, var_off, ref_code,
                                                                                  alt_code, valid);
  return check_launch("ism_variants");
}

// the shift limit of the reduce kernels (reduce.hip: [n_shift][10] f64 in 64 KiB)
constexpr int kIsmMaxShifts = 65536 / (10 * (int)sizeof(double));
constexpr size_t kIsmMaxLds = 160 * 1024;   // gfx950: 160 KiB of LDS per CU; above 64 KiB is an opt-in

int expecto_ism_score(const float* y_ref, const float* y_alt, long long strand_stride, const long long* dist,
                      int strand_plus, const int* shifts, int n_shift, int n, int nfeat, const double* exp_lut,
                      int lut_len, const int* keep, int nk, const float* w, const float* init, int n_models,
                      const uint8_t* valid, float* alt_pred, float* ref_pred, double* sed, void* stream) {
  EXPECTO_REQUIRE(n >= 0 && n_shift > 0 && n_shift <= kIsmMaxShifts && nfeat > 0, "bad shape (n_shift <= 819)");
  EXPECTO_REQUIRE(n % 3 == 0, "n must hold three slots per position (n % 3 == 0)");
  EXPECTO_REQUIRE(nk >= 1 && nk <= nfeat && n_models >= 1, "bad shape (1 <= nk <= nfeat, n_models >= 1)");
  const size_t shm = 30 * (size_t)n_shift * sizeof(double) + (size_t)nk * sizeof(float4);
  EXPECTO_REQUIRE(shm <= kIsmMaxLds, "shifts and kept marks exceed the 160 KiB of LDS");
  if (n == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE((n_models + kIsmThreads - 1) / kIsmThreads <= 65535, "too many models");
  EXPECTO_REQUIRE(strand_stride >= (long long)n_shift * n, "strand_stride below n_shift * n rows");
  EXPECTO_REQUIRE(y_ref && y_alt && dist && shifts && keep && w && init && valid && alt_pred && ref_pred && sed,
                  "null argument");
  EXPECTO_REQUIRE(!exp_lut || lut_len > 0, "empty exp table");
  if (shm > 65536)
    EXPECTO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ism_score_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIsmMaxLds));
  dim3 grid(n / 3, (n_models + kIsmThreads - 1) / kIsmThreads);
  ism_score_kernel<<<grid, dim3(kIsmThreads), shm, as_stream(stream)>>>(
      y_ref, y_alt, strand_stride, dist, strand_plus ? 1 : 0, shifts, n_shift, n, nfeat, exp_lut, lut_len, keep, nk, w,
      init, n_models, valid, alt_pred, ref_pred, sed);
  return check_launch("ism_score");
}

int expecto_ism_summary(const double* sed, const uint8_t* valid, int n_models, int n, double* potential,
                        double* direction, void* stream) {
  EXPECTO_REQUIRE(n_models >= 0 && n >= 0, "negative shape");
  if (n_models == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(potential && direction && (n == 0 || (sed && valid)), "null argument");
  ism_summary_kernel<<<dim3(n_models), dim3(64), 0, as_stream(stream)>>>(sed, valid, n, potential, direction);
  return check_launch("ism_summary");
}

}  // extern "C"
