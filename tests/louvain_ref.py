"""Restatement of the Louvain contract of include/expecto_hip.h (expecto_knn_jaccard, expecto_louvain) and
of ``cluster_and_viz_louvain.symmetrize``: the bits the device must give.  The distances are numpy float64
operations, one per product and per sum; the community search runs on Python floats (IEEE doubles, nothing
fused) in exactly the stated orders.  Also the fixed inputs of the tests and of
tests/golden/make_golden_louvain.py."""
import os

import numpy as np

PASS_BOUND, LEVEL_BOUND, BAD_GRAPH = 1, 2, 4
MIN_GAIN = 1e-7


# ---- the graph -------------------------------------------------------------------------------

def d2(X):
    """[n, n]: s = +0.0; for c ascending t = x_ic - x_jc; s = s + t*t."""
    X = np.asarray(X, np.float64)
    s = np.zeros((X.shape[0], X.shape[0]))
    for c in range(X.shape[1]):
        t = X[:, c, None] - X[None, :, c]
        s = s + t * t
    return s


def knn(X, k):
    """nbr int32 [n, k]: ascending (d2, index); a stable sort keeps the lower index on ties."""
    return np.argsort(d2(X), axis=1, kind="stable")[:, :k].astype(np.int32)


def jaccard(nbr):
    n, k = nbr.shape
    sets = [set(r.tolist()) for r in nbr]
    w = np.zeros((n, k), np.float64)
    for i in range(n):
        for t in range(k):
            j = int(nbr[i, t])
            if j != i:
                both = len(sets[i] & sets[j])
                w[i, t] = np.float64(both) / np.float64(2 * k - both)
    return w


def knn_jaccard(X, k):
    nbr = knn(X, k)
    return nbr, jaccard(nbr)


def symmetrize(nbr, w):
    """CSR (indptr int32, indices int32, weights float64): the edge {i, j}, i != j, where j in N(i) or
    i in N(j); rows ascending in neighbour index."""
    n, k = nbr.shape
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for t in range(k):
            j = int(nbr[i, t])
            if j != i:
                rows[i].setdefault(j, float(w[i, t]))
                rows[j].setdefault(i, float(w[i, t]))
    indptr = np.zeros(n + 1, np.int32)
    indices, weights = [], []
    for i in range(n):
        for j in sorted(rows[i]):
            indices.append(j)
            weights.append(rows[i][j])
        indptr[i + 1] = len(indices)
    return indptr, np.array(indices, np.int32), np.array(weights, np.float64)


def csr_of_networkx(G):
    """A networkx graph with nodes 0..n-1 as CSR, rows ascending, weight 1.0 where none is given."""
    n = G.number_of_nodes()
    indptr = np.zeros(n + 1, np.int32)
    indices, weights = [], []
    for v in range(n):
        for x in sorted(G[v]):
            indices.append(x)
            weights.append(float(G[v][x].get("weight", 1.0)))
        indptr[v + 1] = len(indices)
    return indptr, np.array(indices, np.int32), np.array(weights, np.float64)


# ---- the communities -------------------------------------------------------------------------

def chain(a):
    s = 0.0
    for v in a:
        s = s + v
    return s


def degrees(ptr, idx, w):
    n = len(ptr) - 1
    k = []
    for v in range(n):
        s = 0.0
        for e in range(ptr[v], ptr[v + 1]):
            s = s + (2.0 * w[e] if idx[e] == v else w[e])
        k.append(s)
    return k, chain(k)


def modularity(ptr, idx, w, comm, D, gamma, two_m):
    n = len(ptr) - 1
    L = [0.0] * n
    for v in range(n):
        cv = comm[v]
        s = 0.0
        for e in range(ptr[v], ptr[v + 1]):
            x = idx[e]
            if x >= v and comm[x] == cv:
                s = s + w[e]
        L[cv] = L[cv] + s
    m = two_m * 0.5
    q = 0.0
    for c in range(n):
        r = D[c] / two_m
        q = q + (L[c] / m - gamma * (r * r))
    return q


def gains(ptr, idx, w, comm, D, k, v, gamma, two_m):
    """{slot: gain} of node v, already taken out of D[comm[v]]."""
    old, kv = comm[v], k[v]
    kvc = {}
    for e in range(ptr[v], ptr[v + 1]):
        x = idx[e]
        if x != v:
            c = comm[x]
            kvc[c] = kvc.get(c, 0.0) + w[e]
    if old not in kvc:
        kvc[old] = 0.0
    return {c: s - gamma * D[c] * kv / two_m for c, s in kvc.items()}


def move_pass(ptr, idx, w, comm, D, k, order, gamma, two_m):
    moved = 0
    for v in order:
        old = comm[v]
        D[old] = D[old] - k[v]
        g = gains(ptr, idx, w, comm, D, k, v, gamma, two_m)
        to, best = old, g[old]
        for c in sorted(g):
            if c != old and g[c] > best:
                to, best = c, g[c]
        D[to] = D[to] + k[v]
        comm[v] = to
        moved += to != old
    return moved


def aggregate(ptr, idx, w, comm, labels):
    n = len(ptr) - 1
    newid = {}
    for v in range(n):
        if comm[v] not in newid:
            newid[comm[v]] = len(newid)
    labels = [newid[comm[l]] for l in labels]
    comm = [newid[c] for c in comm]
    members = [[] for _ in newid]
    for v in range(n):
        members[comm[v]].append(v)
    nptr, nidx, nw = [0], [], []
    for C, mem in enumerate(members):
        acc, loop, has_loop = {}, 0.0, False
        for u in mem:
            for e in range(ptr[u], ptr[u + 1]):
                x = idx[e]
                cx = comm[x]
                if cx == C:
                    if x >= u:
                        loop = loop + w[e]
                        has_loop = True
                else:
                    acc[cx] = acc.get(cx, 0.0) + w[e]
        if has_loop:
            acc[C] = loop
        for c in sorted(acc):
            nidx.append(c)
            nw.append(acc[c])
        nptr.append(len(nidx))
    return nptr, nidx, nw, labels


def louvain(indptr, indices, weights, gamma, perm, max_passes=100, max_levels=32):
    """dict: labels int32 [n], modularity float64, n_communities, n_levels, n_passes, flags, and the last
    level's graph (``graph``: ptr, idx, w lists) with its 2m."""
    ptr, idx, w = [int(v) for v in indptr], [int(v) for v in indices], [float(v) for v in weights]
    gamma = float(gamma)
    n = len(ptr) - 1
    labels = list(range(n))
    k, two_m = degrees(ptr, idx, w)
    n_levels = n_passes = flags = 0
    Q = 0.0
    if two_m != 0.0:
        comm, D = list(range(n)), list(k)
        Q = modularity(ptr, idx, w, comm, D, gamma, two_m)
        done = False
        for level in range(max_levels):
            q_start, moved, stop = Q, 0, False
            order = [int(v) for v in perm] if level == 0 else range(len(ptr) - 1)
            for _ in range(max_passes):
                mv = move_pass(ptr, idx, w, comm, D, k, order, gamma, two_m)
                n_passes += 1
                moved += mv
                q = modularity(ptr, idx, w, comm, D, gamma, two_m)
                rise = q - Q
                Q = q
                if mv == 0 or rise < MIN_GAIN:
                    stop = True
                    break
            if not stop:
                flags |= PASS_BOUND
            if moved == 0:
                done = True
                break
            ptr, idx, w, labels = aggregate(ptr, idx, w, comm, labels)
            n_levels += 1
            k, two_m = degrees(ptr, idx, w)
            comm, D = list(range(len(k))), list(k)
            if Q - q_start < MIN_GAIN:
                done = True
                break
        if not done:
            flags |= LEVEL_BOUND
    return dict(labels=np.array(labels, np.int32), modularity=np.float64(Q), n_communities=len(ptr) - 1,
                n_levels=n_levels, n_passes=n_passes, flags=flags, graph=(ptr, idx, w), two_m=two_m)


def permutation(seed, restart, n):
    return np.random.RandomState(seed + restart).permutation(n).astype(np.int32)


def sweep(X, k_neighbors=5, resolutions=(1.0,), n_init=1, seed=0, max_passes=100, max_levels=32):
    """cluster_and_viz_louvain.louvain_sweep by the contract: per resolution the restart of first maximal
    modularity, as (result dict, restart)."""
    nbr, w = knn_jaccard(X, k_neighbors)
    csr = symmetrize(nbr, w)
    out = []
    for gamma in resolutions:
        runs = [louvain(*csr, gamma, permutation(seed, r, len(nbr)), max_passes, max_levels) for r in range(n_init)]
        best = int(np.argmax([r["modularity"] for r in runs]))      # the first maximum
        out.append((runs[best], best))
    return out


# ---- inputs ----------------------------------------------------------------------------------

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "louvain")
CLI_MARKS = 2002


def blobs(n_blobs=5, per=12, d=8, seed=3):
    """The planted blobs: centres RandomState(seed).randn(n_blobs, d) * 20, unit noise; (X, planted labels)."""
    rs = np.random.RandomState(seed)
    centres = rs.randn(n_blobs, d) * 20
    planted = np.repeat(np.arange(n_blobs), per)
    return centres[planted] + rs.randn(n_blobs * per, d), planted


def make_fixture():
    """The fixture's recipe: float32 [2002, 20], 30 overlapping Gaussian groups (make_golden_louvain.py
    stores it as fixture.npz, the tests read the file)."""
    rs = np.random.RandomState(11)
    centres = rs.normal(scale=1.0, size=(30, 20))
    return (centres[rs.randint(30, size=CLI_MARKS)] + rs.normal(size=(CLI_MARKS, 20))).astype(np.float32)


def fixture():
    with np.load(os.path.join(GOLD, "fixture.npz")) as z:
        return z["X"]


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
