"""Plain-Python float64 restatement of the motif similarity clustering (expecto_amd/cluster_by_pwm.py,
csrc/motif_cluster.hip, csrc/average_linkage.h; DESIGN.md "Motif similarity clustering"), so that the
device kernel and the host tree can be compared with it bit for bit.  Nothing here imports the code
under test.

* ``frequencies``: f = (c + pseudo/4) / (((cA + cC) + cG) + cT + pseudo); centred a = f - 0.25.
* ``alignments``: every (strand, offset) of a pair with its three sequential sums (A's columns ascending,
  A C G T within a column, each product rounded before its add), cor and Ncor.
* ``best``: the largest Ncor, ties to strand D, then to the smaller offset.
* ``linkage``: scipy's ``linkage(method='average')``: NN-chain with strict ``<`` and the previous chain
  element preferred, the update evaluated left to right, a stable sort by height, union-find labels.
* ``threshold_cut``: the means over the cross pairs of every merge and the maximal merges that hold.

Also the seeded count matrices that the tests share (``random_counts``, ``special_motifs``, ``planted``)."""
from __future__ import annotations

import math

import numpy as np


# ---- comparison ------------------------------------------------------------------------------

def frequencies(counts, pseudo=1.0):
    """Flat list of 4 w centred values (column-major: A C G T of column 0, ...) of counts [w, 4]."""
    out = []
    for row in np.asarray(counts, np.float64).tolist():
        tot = ((row[0] + row[1]) + row[2]) + row[3]
        for c in row:
            out.append((c + pseudo / 4) / (tot + pseudo) - 0.25)
    return out


def reverse_complement(flat):
    """B_rc[j][b] = B[w-1-j][3-b]: the flat list reversed."""
    return flat[::-1]


def offsets(wA, wB, min_w):
    need = min(min_w, wA, wB)
    return range(-(wB - need), wA - need + 1)


def alignment(A, B, wA, wB, o):
    """(num, ssa, ssb, w) of A against B (already the strand's view) at offset o."""
    lo, hi = max(0, o), min(wA, o + wB)
    num = ssa = ssb = 0.0
    for a, b in zip(A[4 * lo:4 * hi], B[4 * (lo - o):4 * (hi - o)]):
        num = num + a * b
        ssa = ssa + a * a
        ssb = ssb + b * b
    return num, ssa, ssb, hi - lo


def scores(num, ssa, ssb, w, wA, wB):
    den2 = ssa * ssb
    cor = 0.0 if den2 == 0.0 else num / math.sqrt(den2)
    return cor, cor * w / (wA + wB - w)


def alignments(A, B, min_w):
    """Every alignment of two centred flat motifs: (strand, o, w, cor, ncor), D before R per offset."""
    wA, wB = len(A) // 4, len(B) // 4
    views = (B, reverse_complement(B))
    for o in offsets(wA, wB, min_w):
        for s in (0, 1):
            num, ssa, ssb, w = alignment(A, views[s], wA, wB, o)
            cor, ncor = scores(num, ssa, ssb, w, wA, wB)
            yield s, o, w, cor, ncor


def best(A, B, min_w):
    """(cor, ncor, dist, offset, strand, width) of the best alignment."""
    top = None
    for s, o, w, cor, ncor in alignments(A, B, min_w):      # o ascending, D then R
        if top is None or ncor > top[1] or (ncor == top[1] and s < top[4]):
            top = (cor, ncor, max(0.0, 1.0 - ncor), o, s, w)
    return top


def condensed_index(n, i, j):
    if i > j:
        i, j = j, i
    return n * i - i * (i + 1) // 2 + (j - i - 1)


def compare(mats, min_w=5, pseudo=1.0):
    """(cor, ncor, dist float64; offset, strand, width int32) over the pairs in condensed order."""
    flats = [frequencies(m, pseudo) for m in mats]
    M = len(flats)
    rows = [best(flats[i], flats[j], min_w) for i in range(M) for j in range(i + 1, M)]
    cols = list(zip(*rows)) if rows else [()] * 6
    return tuple(np.array(c, np.float64) for c in cols[:3]) + tuple(np.array(c, np.int32) for c in cols[3:])


# ---- tree ------------------------------------------------------------------------------------

def linkage(condensed, n):
    """(children[int64, n-1, 2], heights[float64, n-1], sizes[int64, n-1]) of the condensed matrix."""
    if n < 2:
        raise ValueError("average linkage needs at least 2 points")
    D = [float(v) for v in condensed]
    if any(v != v for v in D):
        raise ValueError("average linkage: NaN in the distance matrix")
    size = [1] * n
    chain, merges = [], []
    for _ in range(n - 1):
        if not chain:
            chain.append(next(i for i in range(n) if size[i] > 0))
        while True:
            x = chain[-1]
            if len(chain) > 1:
                y = chain[-2]
                cur = D[condensed_index(n, x, y)]
            else:
                y, cur = None, math.inf
            for i in range(n):
                if size[i] == 0 or i == x:
                    continue
                d = D[condensed_index(n, x, i)]
                if d < cur:
                    cur, y = d, i
            if y is None:
                raise ValueError("average linkage: a cluster has no neighbour at a finite distance")
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = size[x], size[y]
        merges.append((x, y, cur))
        size[x], size[y] = 0, nx + ny
        for i in range(n):
            if size[i] == 0 or i == y:
                continue
            p = condensed_index(n, i, y)
            D[p] = (float(nx) * D[condensed_index(n, i, x)] + float(ny) * D[p]) / float(nx + ny)
    order = sorted(range(n - 1), key=lambda k: merges[k][2])        # sorted() is stable
    parent = list(range(2 * n - 1))
    usize = [1] * (2 * n - 1)

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
    return children, np.array([merges[m][2] for m in order], np.float64), sizes


def threshold_cut(children, n, cor, ncor, min_cor, min_ncor):
    """(labels[int32, n], mean_cor[float64, n-1], mean_ncor[float64, n-1])."""
    leaves = {v: [v] for v in range(n)}
    accepted = {v: True for v in range(n)}
    up = {}
    mean_cor, mean_ncor = np.empty(n - 1, np.float64), np.empty(n - 1, np.float64)
    for i in range(n - 1):
        a, b = int(children[i][0]), int(children[i][1])
        sc = sn = 0.0
        for x in leaves[a]:
            for y in leaves[b]:
                p = condensed_index(n, x, y)
                sc = sc + float(cor[p])
                sn = sn + float(ncor[p])
        cnt = float(len(leaves[a]) * len(leaves[b]))
        mean_cor[i], mean_ncor[i] = sc / cnt, sn / cnt
        accepted[n + i] = bool(accepted[a] and accepted[b] and mean_cor[i] >= min_cor and mean_ncor[i] >= min_ncor)
        leaves[n + i] = sorted(leaves[a] + leaves[b])
        up[a] = up[b] = n + i
    labels, seen = np.empty(n, np.int32), {}
    for v in range(n):
        top = v
        while top in up and accepted[up[top]]:
            top = up[top]
        labels[v] = seen.setdefault(top, len(seen) + 1)
    return labels, mean_cor, mean_ncor


def cluster(mats, cor=0.6, ncor=0.4, min_w=5, pseudo=1.0):
    """(compare's six arrays, linkage's three, threshold_cut's three)."""
    comp = compare(mats, min_w, pseudo)
    tree = linkage(comp[2], len(mats))
    return comp, tree, threshold_cut(tree[0], len(mats), comp[0], comp[1], cor, ncor)


def clusters_tab(names, labels):
    members = {}
    for name, k in zip(names, labels):
        members.setdefault(int(k), []).append(name)
    return "".join(f"cluster_{k}\t{','.join(members[k])}\n" for k in sorted(members))


def threshold_margin(cut, min_cor, min_ncor):
    """The least distance of a merge's mean from its threshold."""
    return min(float(np.abs(cut[1] - min_cor).min()), float(np.abs(cut[2] - min_ncor).min()))


# ---- shared seeded inputs --------------------------------------------------------------------

def random_counts(w, seed=0, sites=40):
    """Counts float64 [w, 4]: ``sites`` draws per column from a skewed composition; no column is empty."""
    rng = np.random.default_rng([seed, w, 11])
    p = rng.dirichlet(np.full(4, 0.4), w)
    return np.stack([rng.multinomial(sites, q) for q in p]).astype(np.float64)


def rc_counts(c):
    return np.ascontiguousarray(np.asarray(c)[::-1, ::-1])


def gamma_distances(n, seed=0):
    return np.random.default_rng([seed, n, 3]).gamma(0.7, 2.0, n * (n - 1) // 2)


def tie_distances(n, seed=0):
    """Distances from a 4-value set: zero distances and many merges at equal heights."""
    return np.random.default_rng([seed, n, 5]).choice(np.array([0.0, 0.25, 0.5, 1.0]), n * (n - 1) // 2)


def planted(seed=0, per_family=8, singles=9):
    """Three families of jittered copies of three base motifs (widths 8, 10, 12), every other copy reverse
    complemented and every third shifted by a column (one lost at one end, a random one gained at the
    other), plus unrelated random motifs, all shuffled.  Returns (count matrices, names, family of
    each motif: 0..2, or -1 for a singleton)."""
    rng = np.random.default_rng([seed, 20260])
    mats, fam = [], []
    for f, w in enumerate((8, 10, 12)):
        p = rng.dirichlet(np.full(4, 0.12), w)
        p = 0.94 * p + 0.015
        for k in range(per_family):
            c = np.stack([rng.multinomial(200, q) for q in p]).astype(np.float64)
            if k % 3 == 2:
                flank = rng.multinomial(200, rng.dirichlet(np.full(4, 2.0)))[None, :].astype(np.float64)
                c = np.concatenate([c[1:], flank]) if k % 2 else np.concatenate([flank, c[:-1]])
            if k % 2:
                c = rc_counts(c)
            mats.append(c)
            fam.append(f)
    for k in range(singles):
        w = int(rng.integers(6, 14))
        mats.append(np.stack([rng.multinomial(60, q) for q in rng.dirichlet(np.full(4, 0.5), w)]).astype(np.float64))
        fam.append(-1)
    order = rng.permutation(len(mats))
    mats, fam = [mats[i] for i in order], [fam[i] for i in order]
    names = [f"TF{f}_{i}" if f >= 0 else f"ORPHAN{i}" for i, f in enumerate(fam)]
    return mats, names, fam
