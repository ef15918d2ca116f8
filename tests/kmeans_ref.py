"""numpy restatement of the k-means contract of include/expecto_hip.h (expecto_kmeans_plusplus,
expecto_kmeans_lloyd): the bits the device must give.  ``np.cumsum`` and ``np.add.at`` are the
sequential chains; every product and sum is a separate float64 numpy operation, so nothing is fused.
Also the fixed recipe inputs of the sklearn goldens (tests/golden/make_golden_kmeans.py)."""
import numpy as np


def d2(X, C):
    """[n, m]: s = +0.0; for j ascending t = x[j] - c[j]; s = s + t*t."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    s = np.zeros((X.shape[0], C.shape[0]))
    for j in range(X.shape[1]):
        t = X[:, j, None] - C[None, :, j]
        s = s + t * t
    return s


def seq_sum(a):
    a = np.asarray(a, np.float64).ravel()
    return np.float64(np.cumsum(a)[-1]) if a.size else np.float64(0.0)


def trials(k):
    return 2 + int(np.log(k))


def plusplus(X, k, first, u):
    """(idx int32 [k], centres [k, d]); u float64 [k-1, T]."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    u = np.asarray(u, np.float64).reshape(k - 1, -1) if k > 1 else np.empty((0, 1))
    idx = np.empty(k, np.int32)
    idx[0] = first
    closest = d2(X, X[first:first + 1])[:, 0]
    pot = seq_sum(closest)
    for c in range(1, k):
        cum = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cum, u[c - 1] * pot, side="left"), n - 1)
        dc = np.minimum(closest[:, None], d2(X, X[cand]))
        pots = np.cumsum(dc, axis=0)[-1]
        t = int(np.argmin(pots))
        pot, closest, idx[c] = pots[t], np.ascontiguousarray(dc[:, t]), cand[t]
    return idx, X[idx].copy()


def e_step(X, C):
    D = d2(X, C)
    label = np.argmin(D, axis=1).astype(np.int32)
    return label, D[np.arange(X.shape[0]), label]


def m_step(X, C, label, dist):
    """(C_new, shift) of one iteration, relocation included."""
    n, k = X.shape[0], C.shape[0]
    mlab = label.copy()
    empty = np.nonzero(np.bincount(label, minlength=k) == 0)[0]
    if empty.size:
        far = np.lexsort((np.arange(n), -dist))[:empty.size]
        mlab[far] = empty
    count = np.bincount(mlab, minlength=k)
    S = np.zeros_like(C)
    np.add.at(S, mlab, X)
    C_new = C.copy()
    full = count > 0
    C_new[full] = S[full] / count[full, None].astype(np.float64)
    t = (C_new - C).ravel()
    return C_new, seq_sum(t * t)


def lloyd(X, C0, tol, max_iter):
    """(labels int32 [n], centres [k, d], inertia, n_iter)."""
    X, C = np.asarray(X, np.float64), np.array(C0, np.float64)
    prev, strict, n_iter = None, False, 0
    for it in range(max_iter):
        label, dist = e_step(X, C)
        C, shift = m_step(X, C, label, dist)
        n_iter = it + 1
        if prev is not None and np.array_equal(label, prev):
            strict = True
            break
        prev = label
        if shift <= tol:
            break
    if not strict:
        label, _ = e_step(X, C)
    t = X - C[label]
    terms = np.zeros(X.shape[0])
    for j in range(X.shape[1]):
        terms = terms + t[:, j] * t[:, j]
    return label, C, seq_sum(terms), n_iter


def draws(seed, n, ks, n_init):
    """sklearn's draw order (the restatement of cluster_and_viz.kmeans_draws)."""
    rs = np.random.RandomState(seed)
    out = []
    for k in ks:
        T = trials(k)
        per = []
        for _ in range(n_init):
            first = int(rs.choice(n, p=np.full(n, 1.0) / float(n)))
            per.append((first, np.array([rs.uniform(size=T) for _ in range(k - 1)], np.float64).reshape(k - 1, T)))
        out.append(per)
    return out


def tolerance(X, tol=1e-4):
    return float(np.mean(np.var(X, axis=0)) * tol)


def fit(X, k, n_init=1, seed=0, max_iter=300, tol=1e-4):
    """KMeans(k, n_init=n_init, random_state=seed).fit(X) by the contract: dict of the best restart."""
    X = np.asarray(X, np.float64)
    best = None
    for r, (first, u) in enumerate(draws(seed, X.shape[0], [k], n_init)[0]):
        idx, C0 = plusplus(X, k, first, u)
        label, C, inertia, n_iter = lloyd(X, C0, tolerance(X, tol), max_iter)
        if best is None or inertia < best["inertia"]:
            best = dict(labels=label, centres=C, inertia=inertia, n_iter=n_iter, seeds=idx, restart=r)
    return best


# ---- recipe inputs: float32-valued, as tf_idf_reduced_100.npy is, converted to float64 ---------

def blobs(n, d, k, seed):
    rng = np.random.RandomState(seed)
    centres = rng.normal(scale=4.0, size=(k, d))
    X = centres[rng.randint(k, size=n)] + rng.normal(size=(n, d))
    return X.astype(np.float32).astype(np.float64)


def gauss(n, d, seed):
    return np.random.RandomState(seed).normal(size=(n, d)).astype(np.float32).astype(np.float64)


INPUTS = {
    "blobs300": lambda: blobs(300, 5, 7, 100),
    "blobs2002": lambda: blobs(2002, 20, 30, 101),
    "gauss2002": lambda: gauss(2002, 20, 102),
}
# (input, k, n_init) of every recorded case; each with the seeds below
CASES = [("blobs300", 7, 1), ("blobs2002", 30, 1), ("gauss2002", 30, 1), ("gauss2002", 197, 1),
         ("blobs300", 7, 3), ("blobs2002", 30, 3)]
SEEDS = (0, 1, 2)


def case_name(name, k, n_init, seed):
    return f"{name}_k{k}_i{n_init}_s{seed}"


# ---- the reference CLI's fixture -----------------------------------------------------------------

CLI_FLAGS = ["--no_tf_features", "--no_histone_features"]       # the 334 DNase marks stay
CLI_MARKS = 334


def cli_reduced(n_marks):
    """The small ``tf_idf_reduced_100.npy`` of the reference run: float32 [n_marks, 100]."""
    rng = np.random.RandomState(7)
    centres = rng.normal(scale=3.0, size=(30, 100))
    return (centres[rng.randint(30, size=n_marks)] + rng.normal(size=(n_marks, 100))).astype(np.float32)
