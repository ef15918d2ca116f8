"""numpy float64 restatement of the reference's tf-idf + TruncatedSVD of the mark tracks (svd.py:58-85,
svd_transform.py:49-81) and of the Gram route expecto_amd.svd takes, so that the device kernels and
the API can be compared with an oracle where scikit-learn is not installed.  Nothing here imports the
code under test.

X is the track matrix as the per-gene files hold it: [N, marks] float32, column n of the
reference's ``tracks`` is row n here.  With x = X[:, keep] in float64:
    c_n = sum_i x[n,i]   idf_n = log(m / (1 + c_n))   r_i = sum_n x[n,i]   A[i,n] = x[n,i] / r_i * idf_n
* ``fit_exact``: numpy.linalg.svd of A.
* ``fit_gram``: eigh of G = H / (r r^T), H = sum_n t t^T with t = x * idf: the route of the device code.
* ``flip``: sklearn >= 1.5 svd_flip(u_based_decision=False).

Also the seeded inputs the tests share (``tracks``) and the input of the golden run of
tests/golden/make_golden_svd.py (``golden_inputs``)."""
from __future__ import annotations

import functools
import os

import numpy as np

GOLDEN_FILES, GOLDEN_ROWS, GOLDEN_MARKS = 3, 200, 2002


def tracks(marks, files, rows, rank, seed, ratio=0.8, noise=0.5):
    """``files`` arrays [rows, marks] float32: sigmoids of a rank-``rank`` logit whose strengths fall
    geometrically (3 * ratio^j) plus unit noise scaled by ``noise``: separated singular values."""
    rng = np.random.default_rng(seed)
    N = files * rows
    strength = 3.0 * ratio ** np.arange(rank)
    U = rng.normal(size=(N, rank))
    V = rng.normal(size=(marks, rank))
    logit = (U * strength) @ V.T + noise * rng.normal(size=(N, marks)) + rng.normal(size=(1, marks)) - 0.5
    X = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    return [np.ascontiguousarray(X[g * rows:(g + 1) * rows]) for g in range(files)]


def golden_inputs():
    """The three [200, 2002] float32 gene files of the golden run.  The seed is one at which every
    leading component's largest entry stands clear of the runner-up (test_svd_host.py checks it), so
    the sign rule is unambiguous."""
    return tracks(GOLDEN_MARKS, GOLDEN_FILES, GOLDEN_ROWS, rank=24, seed=20280, ratio=0.8)


def golden_names():
    return [f"ENSG{g:05d}.npy" for g in (7, 19, 3)]     # used sorted: input g is the g-th name in sorted order


def write_golden_inputs(root):
    """The golden gene files under ``root``; returns their paths in sorted (column) order."""
    os.makedirs(root, exist_ok=True)
    paths = []
    for name, a in zip(sorted(golden_names()), golden_inputs()):
        np.save(os.path.join(root, name), a)
        paths.append(os.path.join(root, name))
    return paths


def stack(files):
    return np.concatenate([np.asarray(f, np.float32) for f in files], axis=0)


def kept(X, keep):
    return np.asarray(X, np.float32)[:, np.asarray(keep)].astype(np.float64)


def idf(X, keep):
    x = kept(X, keep)
    c = np.zeros(x.shape[0])
    for i in range(x.shape[1]):     # ascending i
        c = c + x[:, i]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x.shape[1] / (1.0 + c))


def rowsum(X, keep):
    return kept(X, keep).sum(axis=0)


def tvalues(X, keep, w=None):
    return kept(X, keep) * (idf(X, keep) if w is None else w)[:, None]


def gram(X, keep, w=None):
    t = tvalues(X, keep, w)
    return t.T @ t


def gram_abs(X, keep, w=None):
    """sum_n |t_i t_j|: the scale of the Gram matrix's rounding-error bound."""
    t = np.abs(tvalues(X, keep, w))
    return t.T @ t


def tfidf(X, keep):
    """A [m, N]: the reference's tf_idf."""
    x = kept(X, keep)
    return (x / x.sum(axis=0)).T * idf(X, keep)[None, :]


def flip(components):
    """Signs [k] making the largest-magnitude entry of every row positive (first on ties)."""
    at = np.argmax(np.abs(components), axis=1)
    s = np.sign(components[np.arange(components.shape[0]), at])
    s[s == 0] = 1.0
    return s


def _finish(A_var, Q, sigma, Vt, m):
    s = flip(Vt)
    X = Q * (sigma * s)[None, :]
    ev = np.var(X, axis=0)
    return {"components_": Vt * s[:, None], "singular_values_": sigma, "x_reduced": X, "explained_variance_": ev,
            "explained_variance_ratio_": ev / A_var}


def fit_exact(X, keep, k):
    """The truncated SVD by numpy.linalg.svd of A in float64, plus ``all_singular_values``."""
    A = tfidf(X, keep)
    U, S, Vt = np.linalg.svd(A, full_matrices=False)
    out = _finish(np.var(A, axis=0).sum(), U[:, :k], S[:k], Vt[:k], A.shape[0])
    out["all_singular_values"] = S
    return out


def fit_gram(X, keep, k):
    """The same by the Gram route: eigh of G = H / (r r^T), components by projection."""
    x = kept(X, keep)
    w, r = idf(X, keep), rowsum(X, keep)
    G = gram(X, keep) / np.outer(r, r)
    m = G.shape[0]
    lam, Q = np.linalg.eigh(G)
    lam, Q = lam[::-1][:k], Q[:, ::-1][:, :k]
    sigma = np.sqrt(lam)
    P = (Q / (sigma[None, :] * r[:, None])).T           # [k, m]
    Vt = (P @ x.T) * w[None, :]
    out = _finish(np.trace(G) / m - G.sum() / (m * m), Q, sigma, Vt, m)
    out["G"] = G
    return out


def project(X, keep, w, P):
    """[k, N] float64: idf_n * sum_i P[c,i] x[n,i]."""
    return (P @ kept(X, keep).T) * w[None, :]


def transform(X, keep, components, w=None, scale=True):
    """[m, k] float64: (1 / r_i) sum_n x[n,i] idf_n V[c,n] (``scale`` False: without the 1 / r_i)."""
    x = kept(X, keep)
    out = tvalues(X, keep, w).T @ np.asarray(components, np.float64).T
    return out / x.sum(axis=0)[:, None] if scale else out


def eig_gaps(all_singular_values, k):
    """Per leading component c < k the smallest gap of lambda_c to a neighbouring eigenvalue (the
    whole spectrum counts: the gap to lambda_k matters for component k-1)."""
    lam = np.asarray(all_singular_values, np.float64) ** 2
    gaps = np.empty(k)
    for c in range(k):
        near = [abs(lam[c] - lam[c - 1])] if c else []
        if c + 1 < lam.size:
            near.append(abs(lam[c] - lam[c + 1]))
        else:
            near.append(lam[c])         # the null space of A A^T lies at 0
        gaps[c] = min(near)
    return gaps


def tolerances(exact, N, k):
    """What the Gram route in float64 may differ from ``fit_exact`` by: (relative error of the
    singular values, per-component error of a unit singular vector).  Forming G costs about
    N * 2^-53 * lambda_1 per entry (64: the constant of the summation and the eigensolver), which
    moves lambda_c by that much and a vector by that over its eigenvalue gap; 2^-22 covers the
    float32 rounding of ``components_``."""
    S = exact["all_singular_values"]
    lam1 = S[0] ** 2
    sv_rel = 64 * 2.0 ** -53 * N * (S[0] / S[k - 1]) ** 2
    vec = 2.0 ** -22 + 64 * 2.0 ** -53 * N * lam1 / eig_gaps(S, k)
    return sv_rel, vec


def row_norms(X, keep):
    """||A[i,:]||_2: the scale of one mark's coordinates' sensitivity to the components' rounding."""
    return np.sqrt((tfidf(X, keep) ** 2).sum(axis=1))


@functools.lru_cache(maxsize=None)
def case(marks, files, rows, rank, seed, k, keep_step=1):
    """(X, keep, fit_exact) of a ``tracks`` input, computed once per process and left unchanged."""
    X = stack(tracks(marks, files, rows, rank, seed))
    keep = np.arange(0, marks, keep_step)
    X.setflags(write=False)
    keep.setflags(write=False)
    return X, keep, fit_exact(X, keep, k)
