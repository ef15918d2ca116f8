// Linear indexing of the tiles of an upper triangle (diagonal tiles included), shared by the kernels
// that compute a symmetric matrix one square tile per workgroup (cluster.hip, svd.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace expecto {

// Tiles per tile-row r of the upper triangle: T - r (columns r .. T-1); tiles before row r.
__device__ inline long long pd_row_start(long long r, long long T) { return r * T - r * (r - 1) / 2; }

// Tile (bi <= bj) of linear upper-triangle tile index t.
__device__ inline void pd_tile_of(long long t, long long T, int& bi, int& bj) {
  const double b = 2.0 * (double)T + 1.0;
  long long r = (long long)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
#pragma unroll
  for (int fix = 0; fix < 2; ++fix) {   // the estimate is within one row of the answer
    if (r > 0 && pd_row_start(r, T) > t) --r;
    if (r < T - 1 && pd_row_start(r + 1, T) <= t) ++r;
  }
  bi = (int)r;
  bj = (int)(r + (t - pd_row_start(r, T)));
}

}  // namespace expecto
