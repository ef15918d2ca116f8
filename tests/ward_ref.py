"""numpy restatement of the Ward clustering the reference runs through sklearn's
AgglomerativeClustering (interpret_features.py:99-120, interpret_features_grouped.py:103-146):
scipy's pdist, its NN-chain Ward linkage and sklearn's tree cut, operation for operation, so that
the device kernel and the host linkage can be compared with it bit for bit where scipy and sklearn
are not installed.  Nothing here imports the code under test.

* ``pdist``: per pair s = 0, then s = s + t*t with t = X[i,k] - X[j,k] for k ascending (product and
  sum rounded separately), sqrt correctly rounded; scipy's condensed order.
* ``linkage``: NN-chain with strict ``<`` and the previous chain element preferred, the Ward update
  evaluated left to right, a stable sort by height, a union-find relabelling.
* ``cut``: sklearn's ``_hc_cut``, labels in the stored order of Python's heap list.

Also the seeded inputs that several tests share (``gamma_points``, ``tie_points``,
``interpret_inputs`` for the golden run of tests/golden/make_golden_interpret.py)."""
from __future__ import annotations

import heapq
import os

import numpy as np


def condensed_index(n, i, j):
    if i > j:
        i, j = j, i
    return n * i - i * (i + 1) // 2 + (j - i - 1)


def pdist(X):
    """Condensed Euclidean distances of the rows of X (float64), summed over k in ascending order."""
    X = np.ascontiguousarray(X, np.float64)
    n, d = X.shape
    out = np.empty(n * (n - 1) // 2, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n - 1):
            s = np.zeros(n - i - 1, np.float64)
            for k in range(d):          # one dimension at a time: numpy never re-associates this sum
                t = X[i, k] - X[i + 1:, k]
                s = s + t * t
            out[condensed_index(n, i, i + 1):condensed_index(n, i, i + 1) + n - i - 1] = np.sqrt(s)
    return out


def linkage(condensed, n):
    """(children[int64, n-1, 2], heights[float64, n-1], sizes[int64, n-1]) of the condensed matrix."""
    if n < 2:
        raise ValueError("ward linkage needs at least 2 points")
    D = np.array(condensed, np.float64)
    if np.isnan(D).any():
        raise ValueError("ward linkage: NaN in the distance matrix")
    # square index table: D[idx[x, i]] is the distance of x and i
    iu = np.triu_indices(n, 1)
    idx = np.zeros((n, n), np.int64)
    idx[iu] = np.arange(D.size)
    idx = idx + idx.T
    size = np.ones(n, np.int64)
    chain = []
    merges = []
    for _ in range(n - 1):
        if not chain:
            chain.append(int(np.nonzero(size)[0][0]))
        while True:
            x = chain[-1]
            if len(chain) > 1:
                y = chain[-2]
                cur = D[idx[x, y]]
            else:
                y, cur = None, np.inf
            act = np.nonzero(size)[0]
            act = act[act != x]
            row = D[idx[x, act]]
            # the scan takes i only when D[x, i] < cur, ascending: the first index of the minimum, if below cur
            if row.size and row.min() < cur:
                y = int(act[np.argmin(row)])
                cur = row.min()
            if y is None:
                raise ValueError("ward linkage: a cluster has no neighbour at a finite distance")
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        merges.append((x, y, cur, nx + ny))
        size[x] = 0
        size[y] = nx + ny
        act = np.nonzero(size)[0]
        act = act[act != y]
        if act.size:
            ni = size[act].astype(np.float64)
            dxi, dyi = D[idx[act, x]], D[idx[act, y]]
            t = 1.0 / (float(nx + ny) + ni)
            with np.errstate(invalid="ignore", over="ignore"):
                D[idx[act, y]] = np.sqrt((ni + nx) * t * dxi * dxi + (ni + ny) * t * dyi * dyi - ni * t * cur * cur)
    h = np.array([m[2] for m in merges], np.float64)
    order = np.argsort(h, kind="stable")
    parent = np.arange(2 * n - 1)
    usize = np.ones(2 * n - 1, np.int64)

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    children = np.empty((n - 1, 2), np.int64)
    sizes = np.empty(n - 1, np.int64)
    for i, m in enumerate(order):
        a, b = sorted((find(merges[m][0]), find(merges[m][1])))
        children[i] = a, b
        parent[a] = parent[b] = n + i
        usize[n + i] = usize[a] + usize[b]
        sizes[i] = usize[n + i]
    return children, h[order], sizes


def ward(X):
    X = np.asarray(X, np.float64)
    return linkage(pdist(X), X.shape[0])


def descendants(node, children, n_leaves):
    out, stack = [], [int(node)]
    while stack:
        v = stack.pop()
        if v < n_leaves:
            out.append(v)
        else:
            stack.extend(int(c) for c in children[v - n_leaves])
    return out


def cut(children, n_leaves, n_clusters):
    """sklearn.cluster._agglomerative._hc_cut."""
    nodes = [-(int(max(children[-1])) + 1)]
    for _ in range(n_clusters - 1):
        these = children[-nodes[0] - n_leaves]
        heapq.heappush(nodes, -int(these[0]))
        heapq.heappushpop(nodes, -int(these[1]))
    label = np.zeros(n_leaves, np.int64)
    for i, node in enumerate(nodes):
        label[descendants(-node, children, n_leaves)] = i
    return label


# ---- shared seeded inputs ------------------------------------------------------------------

def gamma_points(n, d, seed=0):
    """Non-negative, skewed values, as the exp-decay features are."""
    return np.random.default_rng([seed, n, d]).gamma(0.7, 2.0, (n, d))


def tie_points(n, d, seed=0):
    """Integers in {0, 1, 2} with two pairs of exactly duplicated rows: zero distances and many tied
    heights."""
    X = np.random.default_rng([seed, n, d, 7]).integers(0, 3, (n, d)).astype(np.float64)
    X[n // 2] = X[1]
    X[n - 1] = X[n // 3]
    return X


INTERPRET_N_GENES = 40
INTERPRET_N_MARKS = 2002


def interpret_inputs():
    """(X[40, 20020] float64, geneanno text, expression text) of the golden grouped run: genes over
    chr1 / chr8 / chrX (one chrY), one rRNA row, one zero expression value (log 0 with --pseudocount
    0).  Regenerated from the seed wherever it is needed; the 6 MB matrix is not stored."""
    rng = np.random.default_rng(20260)
    n = INTERPRET_N_GENES
    # marks in loose families, so that the tree has structure: family centres plus noise, then the
    # ten exp-decay blocks as scaled, perturbed copies
    fam = rng.integers(0, 25, INTERPRET_N_MARKS)
    centre = rng.gamma(0.7, 1.0, (25, n))
    base = centre[fam].T * rng.uniform(0.5, 2.0, INTERPRET_N_MARKS) + rng.gamma(0.5, 0.15, (n, INTERPRET_N_MARKS))
    blocks = [base * s + rng.gamma(0.5, 0.05, base.shape) for s in np.linspace(1.0, 0.1, 10)]
    X = np.ascontiguousarray(np.concatenate(blocks, axis=1))
    chrom = ["chr1", "chr8", "chrX", "chr1", "chr2"]
    seqnames = [chrom[g % 5] for g in range(n)]
    seqnames[7] = "chrY"
    types = ["protein_coding" if g % 4 else "lincRNA" for g in range(n)]
    types[5] = "rRNA"
    anno = ["id,symbol,seqnames,strand,TSS,CAGE_representative_TSS,type"]
    for g in range(n):
        anno.append(f"ENSG{g:011d},GENE{g},{seqnames[g]},{'+-'[g % 2]},{1000 + 977 * g},{1000 + 977 * g},{types[g]}")
    exp = rng.gamma(1.0, 3.0, (n, 3)).round(3)
    exp[13, 1] = 0.0     # a chr1 gene: dropped from the training rows by the log's finiteness mask alone
    rows = ["tissue_a,tissue_b,tissue_c"] + [",".join(repr(float(v)) for v in r) for r in exp]
    return X, "\n".join(anno) + "\n", "\n".join(rows) + "\n"


def write_interpret_inputs(root):
    """Write the golden run's three input files under ``root``; returns their paths."""
    X, anno, exp = interpret_inputs()
    paths = [os.path.join(root, f) for f in ("Xreducedall.npy", "geneanno.csv", "geneexp.csv")]
    np.save(paths[0], X)
    for p, text in zip(paths[1:], (anno, exp)):
        with open(p, "w") as f:
            f.write(text)
    return paths
