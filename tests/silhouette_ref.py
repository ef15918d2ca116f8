"""numpy restatement of the silhouette arithmetic that include/expecto_hip.h fixes
(expecto_silhouette_node_sums, expecto_silhouette_cuts) and of the sweep planner, built on
``ward_ref.cut``: what sklearn's ``silhouette_samples(D, labels, metric='precomputed')`` computes,
operation for operation, so that the device kernels can be compared with it bit for bit where
sklearn is not installed.  Nothing here imports the code under test.

* node sum: ``S[i] = ((+0.0 + d(i,j1)) + d(i,j2)) + ...`` over the members ascending, one rounded add
  per member (``np.bincount(labels, weights=D[i])``);
* per point: ``a = S_own / (|own| - 1)``, ``b = min`` over the other clusters of ``S_c / |c|``,
  ``s = (b - a) / max(a, b)``, NaN -> +0.0;
* score: ``np.mean`` of the contiguous row of samples.

Also the three seeded inputs of tests/golden/silhouette (``INPUTS``)."""
from __future__ import annotations

import numpy as np

import ward_ref


def square(condensed, n):
    """The square matrix of a condensed one: both triangles, +0.0 on the diagonal."""
    D = np.zeros((n, n), np.float64)
    D[np.triu_indices(n, 1)] = condensed
    return D + D.T


def node_sum(D, members):
    """S[i] over all points i for one node: the members in the order given, one add each (vectorised
    over the points; every point has its own sequential chain)."""
    s = np.zeros(D.shape[0], np.float64)
    for j in members:
        s = s + D[j]
    return s


def samples_of_sums(S, sizes, own):
    """S [k, n] node sums, sizes [k], own [n] (row of S holding each point) -> samples [n]."""
    n = S.shape[1]
    at = np.arange(n)
    sizes = np.asarray(sizes, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = S[own, at] / (sizes[own] - 1).astype(np.float64)
        M = S / sizes[:, None].astype(np.float64)
        M[own, at] = np.inf
        b = M.min(axis=0)
        s = (b - a) / np.maximum(a, b)
    s[np.isnan(s)] = 0.0
    return s


def samples(D, labels):
    """silhouette_samples(D, labels, metric='precomputed') for a square D."""
    values, own = np.unique(np.asarray(labels), return_inverse=True)
    members = [np.nonzero(own == c)[0] for c in range(len(values))]
    S = np.stack([node_sum(D, m) for m in members])
    return samples_of_sums(S, [len(m) for m in members], own)


def score(row):
    return np.mean(np.ascontiguousarray(row, np.float64))


def sweep(children, D, ks):
    """(scores [len(ks)], samples [len(ks), n]) of the cuts ``ward_ref.cut(children, n, k)``.  A node's
    sum is computed once and shared by the cuts that use it (its members do not depend on k)."""
    n = D.shape[0]
    sums = {}
    out = np.empty((len(ks), n), np.float64)
    for c, k in enumerate(ks):
        values, own = np.unique(ward_ref.cut(children, n, k), return_inverse=True)
        rows, sizes = [], []
        for v in range(len(values)):
            m = np.nonzero(own == v)[0]
            key = m.tobytes()
            if key not in sums:
                sums[key] = node_sum(D, m)
            rows.append(sums[key])
            sizes.append(len(m))
        out[c] = samples_of_sums(np.stack(rows), sizes, own)
    return np.array([score(r) for r in out], np.float64), out


def needed_nodes(children, n, ks):
    """The distinct clusters (sorted member tuples) over the cuts ``ks``."""
    seen = set()
    for k in ks:
        lab = ward_ref.cut(children, n, k)
        seen.update(tuple(np.nonzero(lab == v)[0].tolist()) for v in range(k))
    return seen


def same_partition(a, b):
    """Two labellings with the same clusters under other numbers."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


# ---- shared seeded inputs ------------------------------------------------------------------

def triple_points():
    """60 points: 20 distinct ones, each three times in a row -- zero distances, a = b = 0 wherever a
    cut separates duplicates."""
    return np.repeat(ward_ref.gamma_points(20, 7, seed=3), 3, axis=0)


INPUTS = {"gamma": lambda: ward_ref.gamma_points(70, 33), "ties": lambda: ward_ref.tie_points(65, 5),
          "triples": triple_points}
