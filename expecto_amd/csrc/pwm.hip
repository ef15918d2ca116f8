// Motif scan of variant flanks (query_fimo_for_predictions.py:43-57: `fimo --thresh 1 --text`, then the
// rows that overlap the variant, then the best row per motif and sequence), without the text table.
//
// pwm_pvalues_kernel: one workgroup per motif.  The score distribution of the scaled integer matrix is
// built column by column in two LDS buffers of 100 w + 1 doubles.  Every lane gathers: target j sums the
// four letters in the order a sequential scatter over ascending source index would have added them
// (scaled entry descending, then alphabet order), product rounded before the add.  Lane 0 then chains
// the tail sums downwards; all lanes clip at 1 and store, entry 0 as exactly 1.
// pwm_scan_kernel: a workgroup takes PW_SEQS sequences x PW_MOTIFS motifs.  The codes of the sequences
// and a mask of their non-ACGT positions lie in LDS; so does, per motif column i and code c, the pair
// (s[i][c], s[w-1-i][3-c]) packed in one 32-bit word, so one add scores a base on both strands (a sum
// is at most 6400: the halves never carry).  A wave takes one motif at a time, a lane one sequence: the
// table reads of a wave are four neighbouring words.  Integers only up to the one table lookup per
// pair; results leave through an LDS tile so that a sequence's motifs are stored side by side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)

namespace expecto {
namespace {

constexpr int PW_MAX_W = 64;                 // motif columns
constexpr int PW_RANGE = 100;                // scaled entries lie in 0..PW_RANGE
constexpr int PW_MAX_L = 256;                // sequence length of a scan
constexpr int PW_THREADS = 256;
constexpr int PW_SEQS = 64;                  // sequences per workgroup: one per lane
constexpr int PW_MOTIFS = 16;                // motifs per workgroup: four per wave
constexpr int PW_MASK_WORDS = PW_MAX_L / 64 + 1;   // one zero word after the last: a window's bits span two
constexpr long long PW_MAX_M = 65535LL * PW_MOTIFS;
constexpr size_t PW_MAX_LDS = 160 * 1024;

__host__ __device__ inline long long pv_size(long long w) { return PW_RANGE * w + 1; }
__host__ __device__ inline long long pv_offset(long long col, long long m) { return PW_RANGE * col + m; }
// bytes of a sequence row in LDS: a whole, odd number of words, so that 64 rows start in 64 banks
__host__ __device__ inline int seq_stride(int L) { return 4 * (((L + 3) / 4) | 1); }

__device__ __forceinline__ int alphabet_code(int a) { return a == 1 ? 2 : a == 2 ? 1 : a; }   // A C G T -> 0 2 1 3

__global__ __launch_bounds__(PW_THREADS) void pwm_pvalues_kernel(
    const short* __restrict__ pssm, const int* __restrict__ col_ptr, long long M, long long total_cols, double bgA,
    double bgC, double bgG, double bgT, int buf_len, double* __restrict__ tables, long long* __restrict__ pv_ptr,
    long long tables_len) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pw_lds[];
  double* cur = reinterpret_cast<double*>(pw_lds);
  double* nxt = cur + buf_len;
  const int tid = threadIdx.x;
  const long long m = blockIdx.x;
  const long long c0 = col_ptr[m];
  const long long w = (long long)col_ptr[m + 1] - c0;
  // the device copy of col_ptr is not the one the host checked: a motif that does not fit is passed over
  if (c0 < 0 || w < 1 || w > PW_MAX_W || c0 + w > total_cols || pv_size(w) > buf_len) return;
  const long long off = pv_offset(c0, m);
  const int size = (int)pv_size(w);
  if (off + size > tables_len) return;
  if (tid == 0) {
    pv_ptr[m] = off;
    if (m == M - 1) pv_ptr[M] = off + size;
    cur[0] = 1.0;
  }
  __syncthreads();
  const double bg[4] = {bgA, bgC, bgG, bgT};
  for (int i = 0; i < (int)w; ++i) {
    int s[4];
    double f[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int v = pssm[(c0 + i) * 4 + alphabet_code(a)];
      s[a] = v < 0 ? 0 : v > PW_RANGE ? PW_RANGE : v;
      f[a] = bg[a];
    }
#pragma unroll
    for (int a = 1; a < 4; ++a)          // insertion sort, stable: entry descending, then alphabet order
#pragma unroll
      for (int b = a; b > 0; --b)
        if (s[b] > s[b - 1]) {
          const int t = s[b];
          s[b] = s[b - 1];
          s[b - 1] = t;
          const double g = f[b];
          f[b] = f[b - 1];
          f[b - 1] = g;
        }
    const int n_old = PW_RANGE * i + 1, n_new = n_old + PW_RANGE;
    for (int j = tid; j < n_new; j += PW_THREADS) {
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = j - s[q];
        double t = 0.0;
        if (k >= 0 && k < n_old) t = cur[k] * f[q];
        acc = acc + t;
      }
      nxt[j] = acc;
    }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (tid == 0) {                        // pv[j] = pv[j + 1] + pdf[j]: one chain, the loads ahead of the adds
    double acc = 0.0;
    int j = size - 1;
    for (; j >= 7; j -= 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = cur[j - u];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc = (j - u == size - 1) ? t[u] : acc + t[u];
        nxt[j - u] = acc;
      }
    }
    for (; j >= 0; --j) {
      acc = (j == size - 1) ? cur[j] : acc + cur[j];
      nxt[j] = acc;
    }
  }
  __syncthreads();
  for (int j = tid; j < size; j += PW_THREADS) {
    const double v = nxt[j];
    tables[off + j] = (j > 0 && v < 1.0) ? v : 1.0;      // pv[0] = P(score >= 0) is 1: the chain ends within a few ulp of it
  }
}

__global__ __launch_bounds__(PW_THREADS) void pwm_scan_kernel(
    const unsigned char* __restrict__ codes, long long S, int L, long long ld, const int* __restrict__ overlap,
    const short* __restrict__ pssm, const int* __restrict__ col_ptr, long long M, long long total_cols,
    const double* __restrict__ tables, const long long* __restrict__ pv_ptr, long long tables_len,
    int* __restrict__ score_out, int* __restrict__ start_out, unsigned char* __restrict__ strand_out,
    double* __restrict__ pvalue_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pw_seq[];          // [PW_SEQS][seq_stride(L)]
  __shared__ unsigned int pair[PW_MOTIFS * PW_MAX_W * 4];                            // (s[i][c], s[w-1-i][3-c])
  __shared__ unsigned long long bad[PW_SEQS][PW_MASK_WORDS];
  __shared__ int m_col[PW_MOTIFS], m_w[PW_MOTIFS];
  __shared__ int t_score[PW_SEQS][PW_MOTIFS + 1], t_start[PW_SEQS][PW_MOTIFS + 1];
  __shared__ unsigned char t_strand[PW_SEQS][PW_MOTIFS + 4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long s0 = (long long)blockIdx.x * PW_SEQS, m0 = (long long)blockIdx.y * PW_MOTIFS;
  const int LS = seq_stride(L);

  // motifs of the tile: local column offset and width; a motif the unchecked device col_ptr misplaces has width 0
  if (tid < PW_MOTIFS) {
    int w = 0;
    if (m0 + tid < M) {
      const long long c0 = col_ptr[m0 + tid], c1 = col_ptr[m0 + tid + 1];
      if (c0 >= 0 && c1 - c0 >= 1 && c1 - c0 <= PW_MAX_W && c1 <= total_cols) w = (int)(c1 - c0);
    }
    m_w[tid] = w;
  }
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    for (int k = 0; k < PW_MOTIFS; ++k) {
      m_col[k] = at;
      at += m_w[k];
    }
  }
  for (int x = tid; x < PW_SEQS * L; x += PW_THREADS) {
    const int r = x / L, p = x - r * L;
    unsigned char c = 4;
    if (s0 + r < S) c = codes[(s0 + r) * ld + p];
    pw_seq[r * LS + p] = c;
  }
  __syncthreads();
  for (int k = wave; k < PW_MOTIFS; k += PW_THREADS / 64) {
    const int w = m_w[k];
    if (w == 0) continue;
    const short* src = pssm + (long long)col_ptr[m0 + k] * 4;
    for (int x = lane; x < 4 * w; x += 64) {
      const int i = x >> 2, c = x & 3;
      const unsigned int fwd = (unsigned short)src[i * 4 + c], rev = (unsigned short)src[(w - 1 - i) * 4 + (3 - c)];
      pair[(m_col[k] + i) * 4 + c] = fwd | (rev << 16);
    }
  }
  {   // PW_SEQS * 4 mask words of 64 positions, one per thread; the fifth word stays zero
    const int r = tid >> 2, word = tid & 3;
    unsigned long long bits = 0;
    for (int b = 0; b < 64; ++b) {
      const int p = word * 64 + b;
      if (p < L && pw_seq[r * LS + p] >= 4) bits |= 1ULL << b;
    }
    bad[r][word] = bits;
    if (word == 0) bad[r][PW_MASK_WORDS - 1] = 0;
  }
  __syncthreads();

  const int c = (s0 + lane < S) ? overlap[s0 + lane] : 0;
  const unsigned char* seq = pw_seq + lane * LS;
  for (int k = wave; k < PW_MOTIFS; k += PW_THREADS / 64) {
    const int w = m_w[k];
    int best = -1, best_p = -1, best_strand = 0;
    if (w > 0 && w <= L) {
      int lo = 0, hi = L - w;
      if (c >= 0) {
        if (c - w + 1 > lo) lo = c - w + 1;
        if (c < hi) hi = c;
      }
      const unsigned int* tab = pair + m_col[k] * 4;
      const unsigned long long ones = w == 64 ? ~0ULL : (1ULL << w) - 1ULL;
      for (int p = lo; p <= hi; ++p) {
        const int q = p >> 6, sh = p & 63;
        unsigned long long bits = bad[lane][q] >> sh;
        if (sh) bits |= bad[lane][q + 1] << (64 - sh);
        if (bits & ones) continue;
        unsigned int sum = 0;
        for (int i = 0; i < w; ++i) sum += tab[i * 4 + seq[p + i]];
        const int plus = (int)(sum & 0xffffu), minus = (int)(sum >> 16);
        if (plus > best) { best = plus; best_p = p; best_strand = 0; }
        if (minus > best) { best = minus; best_p = p; best_strand = 1; }
      }
    }
    t_score[lane][k] = best;
    t_start[lane][k] = best_p;
    t_strand[lane][k] = (unsigned char)best_strand;
  }
  __syncthreads();
  // a thread stores four neighbouring motifs of one sequence
  const int r = tid >> 2;
  if (s0 + r < S) {
    for (int u = 0; u < 4; ++u) {
      const int k = (tid & 3) * 4 + u;
      const long long m = m0 + k;
      if (m >= M) break;
      const int sc = t_score[r][k];
      double pv = __builtin_nan("");
      if (sc >= 0) {
        const long long at = pv_ptr[m] + sc;
        if (pv_ptr[m] >= 0 && at < tables_len && sc <= PW_RANGE * m_w[k]) pv = tables[at];
      }
      const long long o = (s0 + r) * M + m;
      score_out[o] = sc;
      start_out[o] = t_start[r][k];
      strand_out[o] = t_strand[r][k];
      pvalue_out[o] = pv;
    }
  }
}

// col_ptr as the host holds it: starts at 0, widths in [1, PW_MAX_W]
int check_col_ptr(const char* who, const int* col_ptr_host, long long M) {
  const std::string name(who);
  EXPECTO_REQUIRE(col_ptr_host[0] == 0, name + ": col_ptr[0] != 0");
  for (long long m = 0; m < M; ++m) {
    const long long w = (long long)col_ptr_host[m + 1] - col_ptr_host[m];
    EXPECTO_REQUIRE(w >= 0, name + ": decreasing col_ptr");
    EXPECTO_REQUIRE(w >= 1 && w <= PW_MAX_W,
                    name + ": motif " + std::to_string(m) + " has width " + std::to_string(w) + "; supported are 1..64");
  }
  return EXPECTO_OK;
}

}  // namespace
}  // namespace expecto

using namespace expecto;

extern "C" {

int expecto_pwm_pvalues(const short* pssm, const int* col_ptr_host, const int* col_ptr, long long M,
                        const double* bg_host, double* tables, long long* pv_ptr, long long tables_len, void* stream) {
  EXPECTO_REQUIRE(M >= 0, "pwm_pvalues: negative count");
  if (M == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(M < (1LL << 31), "pwm_pvalues: too many motifs");
  EXPECTO_REQUIRE(pssm && col_ptr_host && col_ptr && bg_host && tables && pv_ptr, "null argument");
  if (int e = check_col_ptr("pwm_pvalues", col_ptr_host, M)) return e;
  const long long total = col_ptr_host[M];
  EXPECTO_REQUIRE(tables_len >= pv_offset(total, M), "pwm_pvalues: tables shorter than the sum of 100 w + 1");
  for (int a = 0; a < 4; ++a)
    EXPECTO_REQUIRE(bg_host[a] > 0.0 && bg_host[a] < 1.0, "pwm_pvalues: a background frequency outside (0, 1)");
  hipStream_t st = as_stream(stream);
  {   // the one host read of the matrix: an entry outside the range would index outside a table
    std::vector<short> host((size_t)total * 4);
    EXPECTO_HIP_CHECK(hipMemcpyAsync(host.data(), pssm, host.size() * sizeof(short), hipMemcpyDeviceToHost, st));
    EXPECTO_HIP_CHECK(hipStreamSynchronize(st));
    for (short v : host) EXPECTO_REQUIRE(v >= 0 && v <= PW_RANGE, "pwm_pvalues: a scaled entry outside 0..100");
  }
  int w_max = 0;
  for (long long m = 0; m < M; ++m) {
    const int w = col_ptr_host[m + 1] - col_ptr_host[m];
    if (w > w_max) w_max = w;
  }
  const int buf_len = (int)pv_size(w_max);
  const size_t lds = 2 * (size_t)buf_len * sizeof(double);
  EXPECTO_REQUIRE(lds <= PW_MAX_LDS, "pwm_pvalues: the tables exceed the 160 KiB of LDS");
  if (lds > 65536)
    EXPECTO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pwm_pvalues_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(2 * pv_size(PW_MAX_W) * sizeof(double))));
  // bg arrives in code order (A G C T); the sums run in alphabet order
  pwm_pvalues_kernel<<<dim3((unsigned)M), dim3(PW_THREADS), lds, st>>>(pssm, col_ptr, M, total, bg_host[0], bg_host[2],
                                                                       bg_host[1], bg_host[3], buf_len, tables, pv_ptr,
                                                                       tables_len);
  return check_launch("pwm_pvalues");
}

int expecto_pwm_scan(const unsigned char* codes, long long S, long long L, long long ld, const int* overlap,
                     const short* pssm, const int* col_ptr_host, const int* col_ptr, long long M, const double* tables,
                     const long long* pv_ptr, long long tables_len, int* score, int* start, unsigned char* strand,
                     double* pvalue, void* stream) {
  EXPECTO_REQUIRE(S >= 0 && M >= 0, "pwm_scan: negative count");
  EXPECTO_REQUIRE(L >= 1 && L <= PW_MAX_L, "pwm_scan: L must lie in [1, 256]");
  EXPECTO_REQUIRE(ld >= L, "pwm_scan: row stride ld < L");
  EXPECTO_REQUIRE(M <= PW_MAX_M, "pwm_scan: at most 1048560 motifs per call");
  EXPECTO_REQUIRE((S + PW_SEQS - 1) / PW_SEQS < (1LL << 31), "pwm_scan: too many sequences");
  if (S == 0 || M == 0) return EXPECTO_OK;
  EXPECTO_REQUIRE(codes && overlap && pssm && col_ptr_host && col_ptr && tables && pv_ptr && score && start && strand &&
                      pvalue,
                  "null argument");
  if (int e = check_col_ptr("pwm_scan", col_ptr_host, M)) return e;
  EXPECTO_REQUIRE(tables_len >= pv_offset(col_ptr_host[M], M), "pwm_scan: tables shorter than the sum of 100 w + 1");
  const size_t lds = (size_t)PW_SEQS * seq_stride((int)L);
  pwm_scan_kernel<<<dim3((unsigned)((S + PW_SEQS - 1) / PW_SEQS), (unsigned)((M + PW_MOTIFS - 1) / PW_MOTIFS)),
                    dim3(PW_THREADS), lds, as_stream(stream)>>>(codes, S, (int)L, ld, overlap, pssm, col_ptr, M,
                                                                col_ptr_host[M], tables, pv_ptr, tables_len, score, start,
                                                                strand, pvalue);
  return check_launch("pwm_scan");
}

}  // extern "C"
