// Ward linkage of a condensed distance matrix on the host: scipy's linkage(method='ward'), i.e. the
// NN-chain algorithm, a stable sort of the merges by height and a union-find relabelling
// (interpret_features.py:99-107 through sklearn's AgglomerativeClustering, whose unstructured Ward
// path is scipy.cluster.hierarchy.ward).  Plain C++17, no HIP: cluster.hip includes it for the C
// entry point and tests/ward_linkage_driver.cpp builds it with the host compiler alone.
//
// The arithmetic is scipy's, operation for operation, so the tree equals scipy's bit for bit:
// every product and sum below is rounded on its own (contraction off) and evaluated left to right.
#pragma once

#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif   // GCC has no such pragma: build with -ffp-contract=off (its default under -std=c++17)

namespace expecto {

enum { WARD_OK = 0, WARD_ESIZE = 1, WARD_ENAN = 2, WARD_ENEIGHBOUR = 3 };

inline const char* ward_error_text(int status) {
  switch (status) {
    case WARD_OK: return "";
    case WARD_ESIZE: return "ward linkage needs at least 2 points";
    case WARD_ENAN: return "ward linkage: NaN in the distance matrix";
    case WARD_ENEIGHBOUR: return "ward linkage: a cluster has no neighbour at a finite distance";
    default: return "ward linkage: unknown status";
  }
}

// Index of pair (i, j), i != j, in scipy's condensed order.
inline long long ward_condensed_index(long long n, long long i, long long j) {
  if (i > j) std::swap(i, j);
  return n * i - i * (i + 1) / 2 + (j - i - 1);
}

// condensed: n(n-1)/2 distances, overwritten.  children [n-1][2], heights [n-1], sizes [n-1]: row i is
// the i-th merge by height; it forms cluster n + i out of children[i] (smaller id first).
inline int ward_linkage(double* D, int n, int* children, double* heights, int* sizes) {
  if (n < 2) return WARD_ESIZE;
  const long long npair = (long long)n * (n - 1) / 2;
  for (long long p = 0; p < npair; ++p)
    if (D[p] != D[p]) return WARD_ENAN;

  struct Merge { int x, y; double h; };
  std::vector<Merge> merges((size_t)n - 1);
  std::vector<int> size((size_t)n, 1), chain((size_t)n);
  int chain_len = 0;

  for (int k = 0; k < n - 1; ++k) {
    if (chain_len == 0) {
      for (int i = 0; i < n; ++i)
        if (size[i] > 0) { chain[0] = i; break; }
      chain_len = 1;
    }
    int x, y;
    double cur;
    for (;;) {   // follow nearest neighbours until two clusters are each other's
      x = chain[chain_len - 1];
      if (chain_len > 1) {   // the previous element wins ties, so the chain cannot cycle
        y = chain[chain_len - 2];
        cur = D[ward_condensed_index(n, x, y)];
      } else {
        y = -1;
        cur = std::numeric_limits<double>::infinity();
      }
      for (int i = 0; i < n; ++i) {
        if (size[i] == 0 || i == x) continue;
        const double dist = D[ward_condensed_index(n, x, i)];
        if (dist < cur) { cur = dist; y = i; }
      }
      if (y < 0) return WARD_ENEIGHBOUR;   // every distance from x is +inf
      if (chain_len > 1 && y == chain[chain_len - 2]) break;
      chain[chain_len++] = y;
    }
    if (cur != cur) return WARD_ENAN;   // an update rounded below zero under its sqrt; the sort needs an order
    chain_len -= 2;
    if (x > y) std::swap(x, y);
    const int nx = size[x], ny = size[y];
    merges[k] = {x, y, cur};
    size[x] = 0;         // x is dropped, the merged cluster lives at y
    size[y] = nx + ny;
    for (int i = 0; i < n; ++i) {
      const int ni = size[i];
      if (ni == 0 || i == y) continue;
      const double dxi = D[ward_condensed_index(n, i, x)];
      double& dyi = D[ward_condensed_index(n, i, y)];
      const double t = 1.0 / (double)(nx + ny + ni);
      dyi = std::sqrt((double)(ni + nx) * t * dxi * dxi + (double)(ni + ny) * t * dyi * dyi -
                      (double)ni * t * cur * cur);
    }
  }

  std::vector<int> order((size_t)n - 1);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return merges[a].h < merges[b].h; });

  std::vector<int> parent((size_t)2 * n - 1), usize((size_t)2 * n - 1, 1);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int v) {
    int p = v;
    while (parent[v] != v) v = parent[v];
    while (parent[p] != v) { const int q = parent[p]; parent[p] = v; p = q; }
    return v;
  };
  for (int i = 0; i < n - 1; ++i) {
    const Merge& m = merges[order[i]];
    int a = find(m.x), b = find(m.y);
    if (a > b) std::swap(a, b);
    children[2 * i] = a;
    children[2 * i + 1] = b;
    heights[i] = m.h;
    parent[a] = parent[b] = n + i;
    usize[n + i] = usize[a] + usize[b];
    sizes[i] = usize[n + i];
  }
  return WARD_OK;
}

}  // namespace expecto
