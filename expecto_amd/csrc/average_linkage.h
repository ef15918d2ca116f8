// Average linkage (UPGMA) of a condensed distance matrix on the host, and the cut of such a tree by
// two thresholds on the mean pairwise scores of every merge: the tree and the clusters of
// cluster_by_pwm (DESIGN.md "Motif similarity clustering").  Plain C++17, no HIP: motif_cluster.hip
// includes it for the C entry points and tests/average_linkage_driver.cpp builds it with the host
// compiler alone.
//
// average_linkage is scipy's linkage(method='average') operation for operation, as ward_linkage.h is
// its Ward: the NN-chain algorithm with the update (n_x d_xi + n_y d_yi) / (n_x + n_y), a stable
// sort of the merges by height and a union-find relabelling.  Every product and sum is rounded on its
// own (contraction off) and evaluated left to right, so the tree equals scipy's bit for bit.
#pragma once

#include <algorithm>
#include <limits>
#include <numeric>
#include <utility>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif   // GCC has no such pragma: build with -ffp-contract=off (its default under -std=c++17)

namespace expecto {

enum { AVG_OK = 0, AVG_ESIZE = 1, AVG_ENAN = 2, AVG_ENEIGHBOUR = 3, AVG_ETREE = 4 };

inline const char* average_error_text(int status) {
  switch (status) {
    case AVG_OK: return "";
    case AVG_ESIZE: return "average linkage needs at least 2 points";
    case AVG_ENAN: return "average linkage: NaN in the distance matrix";
    case AVG_ENEIGHBOUR: return "average linkage: a cluster has no neighbour at a finite distance";
    case AVG_ETREE: return "threshold cut: children is not a tree of n leaves (merge i joins two unused nodes below n + i)";
    default: return "average linkage: unknown status";
  }
}

// Index of pair (i, j), i != j, in scipy's condensed order.
inline long long avg_condensed_index(long long n, long long i, long long j) {
  if (i > j) std::swap(i, j);
  return n * i - i * (i + 1) / 2 + (j - i - 1);
}

// condensed: n(n-1)/2 distances, overwritten.  children [n-1][2], heights [n-1], sizes [n-1]: row i is
// the i-th merge by height; it forms cluster n + i out of children[i] (smaller id first).
inline int average_linkage(double* D, int n, int* children, double* heights, int* sizes) {
  if (n < 2) return AVG_ESIZE;
  const long long npair = (long long)n * (n - 1) / 2;
  for (long long p = 0; p < npair; ++p)
    if (D[p] != D[p]) return AVG_ENAN;

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
        cur = D[avg_condensed_index(n, x, y)];
      } else {
        y = -1;
        cur = std::numeric_limits<double>::infinity();
      }
      for (int i = 0; i < n; ++i) {
        if (size[i] == 0 || i == x) continue;
        const double dist = D[avg_condensed_index(n, x, i)];
        if (dist < cur) { cur = dist; y = i; }
      }
      if (y < 0) return AVG_ENEIGHBOUR;   // every distance from x is +inf
      if (chain_len > 1 && y == chain[chain_len - 2]) break;
      chain[chain_len++] = y;
    }
    if (cur != cur) return AVG_ENAN;   // inf - inf in an update; the sort needs an order
    chain_len -= 2;
    if (x > y) std::swap(x, y);
    const int nx = size[x], ny = size[y];
    merges[k] = {x, y, cur};
    size[x] = 0;         // x is dropped, the merged cluster lives at y
    size[y] = nx + ny;
    for (int i = 0; i < n; ++i) {
      if (size[i] == 0 || i == y) continue;
      const double dxi = D[avg_condensed_index(n, i, x)];
      double& dyi = D[avg_condensed_index(n, i, y)];
      dyi = ((double)nx * dxi + (double)ny * dyi) / (double)(nx + ny);
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
  return AVG_OK;
}

// The clusters of a tree under two thresholds.  children [n-1][2] as average_linkage writes it; cor
// and ncor: n(n-1)/2 pairwise scores in condensed order.  For merge i of the clusters X = children[i][0]
// and Y = children[i][1], mean_cor[i] is s = +0.0, then s = s + cor[x, y] over X's leaves ascending
// (outer) and Y's leaves ascending (inner), then s / (double)(|X| |Y|); mean_ncor[i] likewise.  The
// merge is accepted when both children are leaves or accepted merges and mean_cor[i] >= min_cor and
// mean_ncor[i] >= min_ncor (a NaN mean is never accepted).  The clusters are the maximal accepted
// nodes and the leaves under no accepted merge; labels [n] are 1-based, numbered by ascending
// smallest member index.
inline int linkage_threshold_cut(const int* children, int n, const double* cor, const double* ncor, double min_cor,
                                 double min_ncor, int* labels, double* mean_cor, double* mean_ncor) {
  if (n < 2) return AVG_ESIZE;
  const int nodes = 2 * n - 1;
  std::vector<int> up((size_t)nodes, -1);
  for (int i = 0; i < n - 1; ++i)
    for (int c = 0; c < 2; ++c) {
      const int v = children[2 * i + c];
      if (v < 0 || v >= n + i || up[v] >= 0) return AVG_ETREE;
      up[v] = n + i;
    }
  std::vector<std::vector<int>> leaves((size_t)nodes);
  for (int v = 0; v < n; ++v) leaves[v].assign(1, v);
  std::vector<char> accepted((size_t)nodes, 0);
  for (int v = 0; v < n; ++v) accepted[v] = 1;
  for (int i = 0; i < n - 1; ++i) {
    const int a = children[2 * i], b = children[2 * i + 1];
    const std::vector<int>&X = leaves[a], &Y = leaves[b];
    double sc = 0.0, sn = 0.0;
    for (int x : X)
      for (int y : Y) {
        const long long p = avg_condensed_index(n, x, y);
        sc = sc + cor[p];
        sn = sn + ncor[p];
      }
    const double cnt = (double)((long long)X.size() * (long long)Y.size());
    mean_cor[i] = sc / cnt;
    mean_ncor[i] = sn / cnt;
    accepted[n + i] = accepted[a] && accepted[b] && mean_cor[i] >= min_cor && mean_ncor[i] >= min_ncor;
    std::vector<int>& Z = leaves[n + i];
    Z.resize(X.size() + Y.size());
    std::merge(X.begin(), X.end(), Y.begin(), Y.end(), Z.begin());
    std::vector<int>().swap(leaves[a]);   // a node's list is needed once, by its parent
    std::vector<int>().swap(leaves[b]);
  }
  std::vector<int> label_of((size_t)nodes, 0);
  int next = 0;
  for (int v = 0; v < n; ++v) {   // ascending leaves: a cluster is numbered when its smallest member is met
    int top = v;
    while (up[top] >= 0 && accepted[up[top]]) top = up[top];
    if (label_of[top] == 0) label_of[top] = ++next;
    labels[v] = label_of[top];
  }
  return AVG_OK;
}

}  // namespace expecto
