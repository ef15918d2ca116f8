"""Drop-in for the reference ``cluster_and_viz.py``: k-means of the marks' SVD coordinates
(``tf_idf_reduced_100.npy`` of ``expecto_amd.svd``) on the GPU, and the cluster files that
``predict_by_cluster --feature_clusters_df`` reads.

    python -m expecto_amd.cluster_and_viz <svd_transform_dir> --belugaFeatures features.tsv [ablation flags] \\
        [-o temp_cluster_and_viz] [--n_pcs 20] [--n_clusters 30] [--n_init 1] [--seed 0] [--elbow K_MIN K_MAX STEP]

The reference runs ``KMeans(n_clusters=30)`` after ``np.random.seed(0)`` on the first 20 coordinates.
Here the seeding (sklearn's greedy k-means++) and the Lloyd iteration run on the device
(``expecto_kmeans_plusplus``, ``expecto_kmeans_lloyd``) in float64 with a fixed order of every sum
(include/expecto_hip.h); the random numbers are drawn on the host in sklearn's order
(:func:`kmeans_draws`), so ``--seed 0`` consumes the stream the reference consumes.  ``--elbow`` is the
sweep the reference has commented out (``for k in range(2, 200, 5)``): every ``(k, restart)`` is one
problem of a single seeding call and a single Lloyd call.

Differences from the reference, on purpose:
* float64 arithmetic on the file's float32 values (sklearn computes in float32 through BLAS there);
* no t-SNE and no scatter plot: a picture that nothing downstream reads;
* ``--intersect_with_lambert`` and ``--no_pol2`` of cluster_utils are accepted, as in ``svd.py``;
* a ``.npy`` whose row count differs from the number of kept marks is refused with a message (the
  reference dies with a pandas length error).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import NamedTuple

import numpy as np

N_PCS = 20          # cluster_and_viz.py:39
N_CLUSTERS = 30     # cluster_and_viz.py:55
MAX_N, MAX_D, MAX_K = 4096, 128, 512     # include/expecto_hip.h
_COLS = 8


class KMeansResult(NamedTuple):
    labels: np.ndarray        # int32 [n]
    centres: np.ndarray       # float64 [k, d]
    inertia: float
    n_iter: int
    seeds: np.ndarray         # int32 [k]: the k-means++ point indices of the winning restart
    restart: int              # the winning restart: the first of minimal inertia


def trials(k: int) -> int:
    """sklearn's n_local_trials."""
    return 2 + int(np.log(k))


def kmeans_draws(seed, n: int, ks, n_init: int = 1):
    """The host random numbers of ``KMeans(k, n_init=n_init, random_state=seed)`` in sklearn's draw order,
    from one ``np.random.RandomState(seed)``: for each k in the order given and each restart, the first
    centre ``rs.choice(n, p=1/n)`` and then k-1 times ``rs.uniform(size=T)``.  Returns, per k, a list of
    ``(first, u float64 [k-1, T])`` per restart."""
    rs = np.random.RandomState(seed)
    out = []
    for k in ks:
        k = int(k)
        T = trials(k)
        per = []
        for _ in range(int(n_init)):
            first = int(rs.choice(n, p=np.full(n, 1.0) / float(n)))
            u = np.empty((k - 1, T), np.float64)
            for c in range(k - 1):
                u[c] = rs.uniform(size=T)
            per.append((first, u))
        out.append(per)
    return out


def _checked(X, ks, n_init):
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if X.ndim != 2:
        raise ValueError(f"kmeans: X must be 2-D, got shape {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError("kmeans: X contains NaN or infinity")
    n, d = X.shape
    if not (1 <= n <= MAX_N and 1 <= d <= MAX_D):
        raise ValueError(f"kmeans: X has shape {X.shape}; supported are 1..{MAX_N} points of 1..{MAX_D} dimensions")
    ks = [int(k) for k in ks]
    for k in ks:
        if not 1 <= k <= min(n, MAX_K):
            raise ValueError(f"kmeans: n_clusters = {k} outside [1, min(n, {MAX_K})] with n = {n}")
    if int(n_init) < 1:
        raise ValueError("kmeans: n_init must be at least 1")
    return X, ks


def _table(rows):
    t = np.zeros((len(rows), _COLS), np.int64)
    for p, r in enumerate(rows):
        t[p, :len(r)] = r
    return t


def run_problems(X, problems, tol, max_iter, device=None, timings=None):
    """Seed and iterate ``problems`` = [(k, first, u [k-1, T])] on X (float64 [n, d], host) in one
    ``expecto_kmeans_plusplus`` and one ``expecto_kmeans_lloyd`` call.  Returns per problem
    ``(labels, centres, inertia, n_iter, seeds)``.  ``timings``: a dict that receives the two calls'
    device times in ms (``seeding_ms``, ``lloyd_ms``), measured with events."""
    import torch

    from . import _lib
    if not torch.cuda.is_available():
        raise RuntimeError("expecto_amd.cluster_and_viz needs a GPU (HIP); there is no CPU path")
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n, d = X.shape
    P = len(problems)
    if P == 0:
        return []
    ks = np.array([p[0] for p in problems], np.int64)
    Ts = np.array([max(1, np.asarray(p[2]).reshape(p[0] - 1, -1).shape[1]) if p[0] > 1 else 1 for p in problems],
                  np.int64)
    c_off = np.concatenate([[0], np.cumsum(ks)])
    u_off = np.concatenate([[0], np.cumsum((ks - 1) * Ts)])
    seed_tab = _table([(k, p[1], T, u_off[i], c_off[i], c_off[i]) for i, (p, k, T) in enumerate(zip(problems, ks, Ts))])
    lloyd_tab = _table([(k, max_iter, c_off[i], c_off[i], i * n) for i, k in enumerate(ks)])
    u = np.concatenate([np.asarray(p[2], np.float64).ravel() for p in problems] + [np.zeros(1)])
    nbytes = int(lib.expecto_kmeans_workspace(n, d, int(ks.max()), int(Ts.max()), P))

    def call(name, *args):
        st = getattr(lib, name)(*args, _lib.stream_ptr())
        if st != 0:
            raise RuntimeError(f"{name} failed (status {st}): {lib.expecto_last_error().decode()}")

    with torch.cuda.device(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        Xd, ud, seed_d, lloyd_d = up(X), up(u), up(seed_tab), up(lloyd_tab)
        told = torch.full((P,), float(tol), dtype=torch.float64, device=dev)
        total = int(c_off[-1])
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        init = torch.empty((total, d), dtype=torch.float64, device=dev)
        centres = torch.empty((total, d), dtype=torch.float64, device=dev)
        labels = torch.empty((P, n), dtype=torch.int32, device=dev)
        inertia = torch.empty(P, dtype=torch.float64, device=dev)
        n_iter = torch.empty(P, dtype=torch.int32, device=dev)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
        if ev:
            ev[0].record()
        call("expecto_kmeans_plusplus", Xd.data_ptr(), n, d, d, P, seed_tab.ctypes.data, seed_d.data_ptr(),
             ud.data_ptr(), idx.data_ptr(), init.data_ptr(), ws.data_ptr(), nbytes)
        if ev:
            ev[1].record()
        call("expecto_kmeans_lloyd", Xd.data_ptr(), n, d, d, P, lloyd_tab.ctypes.data, lloyd_d.data_ptr(),
             told.data_ptr(), init.data_ptr(), labels.data_ptr(), centres.data_ptr(), inertia.data_ptr(),
             n_iter.data_ptr(), ws.data_ptr(), nbytes)
        if ev:
            ev[2].record()
        idx, centres, labels = idx.cpu().numpy(), centres.cpu().numpy(), labels.cpu().numpy()
        inertia, n_iter = inertia.cpu().numpy(), n_iter.cpu().numpy()
        if ev:
            timings["seeding_ms"] = ev[0].elapsed_time(ev[1])
            timings["lloyd_ms"] = ev[1].elapsed_time(ev[2])
    return [(labels[i], centres[c_off[i]:c_off[i + 1]].copy(), float(inertia[i]), int(n_iter[i]),
             idx[c_off[i]:c_off[i + 1]].copy()) for i in range(P)]


def tolerance(X, tol: float) -> float:
    """sklearn's ``_tolerance``: the relative ``tol`` scaled by the mean variance of the columns."""
    return float(np.mean(np.var(X, axis=0)) * tol)


def kmeans_sweep(X, ks, n_init: int = 1, seed=0, max_iter: int = 300, tol: float = 1e-4, device=None, timings=None):
    """``KMeans(k, n_init=n_init, random_state=seed).fit(X)`` for every k of ``ks``: all ``(k, restart)``
    problems in one seeding call and one Lloyd call.  Each k draws from a fresh ``RandomState(seed)``, so
    its result equals :func:`kmeans` of that k alone.  Returns a list of :class:`KMeansResult`."""
    X, ks = _checked(X, ks, n_init)
    if int(max_iter) < 1:
        raise ValueError("kmeans: max_iter must be at least 1")
    problems = []
    for k in ks:
        for first, u in kmeans_draws(seed, X.shape[0], [k], n_init)[0]:
            problems.append((k, first, u))
    res = run_problems(X, problems, tolerance(X, tol), int(max_iter), device=device, timings=timings)
    out = []
    for i, k in enumerate(ks):
        per = res[i * n_init:(i + 1) * n_init]
        r = int(np.argmin([p[2] for p in per]))       # the first of minimal inertia
        out.append(KMeansResult(per[r][0], per[r][1], per[r][2], per[r][3], per[r][4], r))
    return out


def kmeans(X, k: int, n_init: int = 1, seed=0, max_iter: int = 300, tol: float = 1e-4, device=None) -> KMeansResult:
    """``KMeans(k, n_init=n_init, random_state=seed).fit(X)`` on the device: labels, centres, inertia,
    n_iter, the seeding indices and the winning restart.  X is converted to float64; ``ValueError`` for
    non-finite input, before the device is touched."""
    return kmeans_sweep(X, [k], n_init=n_init, seed=seed, max_iter=max_iter, tol=tol, device=device)[0]


# ---- CLI -------------------------------------------------------------------------------------

def build_parser():
    """The arguments of cluster_and_viz.py:13-28, cluster_utils' two further filters, and the knobs the
    reference has as constants."""
    parser = argparse.ArgumentParser(prog="python -m expecto_amd.cluster_and_viz",
                                     description='Cluster SVD-transformed data')
    parser.add_argument('svd_transform_dir')
    parser.add_argument('--belugaFeatures', action="store", dest="belugaFeatures", required=True,
                        help="tsv file denoting Beluga features")
    parser.add_argument('--no_tf_features', action='store_true', dest='no_tf_features', default=False,
                        help='leave out TF marks for training')
    parser.add_argument('--no_dnase_features', action='store_true', dest='no_dnase_features', default=False,
                        help='leave out DNase marks for training')
    parser.add_argument('--no_histone_features', action='store_true', dest='no_histone_features', default=False,
                        help='leave out histone marks for training')
    parser.add_argument('--intersect_with_lambert', action='store_true', dest='intersect_with_lambert', default=False,
                        help='intersect with Lambert2018_TFs_v_1.01_curatedTFs.csv')
    parser.add_argument('--no_pol2', action='store_true', dest='no_pol2', default=False, help='take out Pol2*')
    parser.add_argument('-o', dest="out_dir", type=str, default='temp_cluster_and_viz', help='Output directory')
    parser.add_argument('--n_pcs', type=int, default=N_PCS, help='leading SVD coordinates to cluster on')
    parser.add_argument('--n_clusters', type=int, default=N_CLUSTERS)
    parser.add_argument('--n_init', type=int, default=1, help='k-means++ restarts; the best inertia is kept')
    parser.add_argument('--seed', type=int, default=0, help='seed of the host random stream')
    parser.add_argument('--elbow', type=int, nargs=3, metavar=('K_MIN', 'K_MAX', 'STEP'), default=None,
                        help='also fit every k of range(K_MIN, K_MAX, STEP) and write elbow.tsv')
    return parser


def run(args):
    import pandas as pd

    from . import predict

    os.makedirs(args.out_dir, exist_ok=True)
    X = np.load(f'{args.svd_transform_dir}/tf_idf_reduced_100.npy')
    if X.ndim != 2 or not 1 <= args.n_pcs <= X.shape[1]:
        raise ValueError(f"tf_idf_reduced_100.npy has shape {X.shape}; --n_pcs {args.n_pcs} needs [marks, >= n_pcs]")
    X = X[:, :args.n_pcs]
    print("clustering...")

    beluga_features_df = predict.read_features_table(args.belugaFeatures)
    keep_mask, _ = predict.get_keep_mask(beluga_features_df, *predict.mask_arguments(args), return_hgnc_df=True)
    keep_mask = np.asarray(keep_mask)
    n_keep = int(keep_mask.sum())
    if X.shape[0] != n_keep:
        raise ValueError(f"tf_idf_reduced_100.npy has {X.shape[0]} rows, the ablation flags of this run keep "
                         f"{n_keep} marks of {args.belugaFeatures}")

    k = args.n_clusters
    if args.elbow is not None:
        ks = list(range(*args.elbow))
        if not ks:
            raise ValueError(f"--elbow {args.elbow[0]} {args.elbow[1]} {args.elbow[2]}: an empty range")
        swept = kmeans_sweep(X, ks, n_init=args.n_init, seed=args.seed)
        with open(f'{args.out_dir}/elbow.tsv', 'w') as f:
            f.write('k\tinertia\tn_iter\trestart\n')
            f.writelines(f'{kk}\t{r.inertia!r}\t{r.n_iter}\t{r.restart}\n' for kk, r in zip(ks, swept))

    result = kmeans(X, k, n_init=args.n_init, seed=args.seed)
    labels = result.labels

    # Save clustering (cluster_and_viz.py:69-103)
    input_features_df = beluga_features_df[keep_mask].copy()
    input_features_df['cluster'] = labels
    input_features_df.to_csv(f'{args.out_dir}/all_feature_clusters.tsv', sep='\t')

    cluster_dir = f'{args.out_dir}/clusters'
    os.makedirs(cluster_dir, exist_ok=True)
    sizes_df = pd.DataFrame(columns=['size'])
    for i in range(k):
        cluster_df = input_features_df[input_features_df['cluster'] == i]
        cluster_df.to_csv(f'{cluster_dir}/cluster_{i}.tsv', sep='\t')
        sizes_df.loc[f'cluster_{i}'] = cluster_df.shape[0]
    sizes_df = sizes_df.sort_values(by='size', ascending=False)
    sizes_df.to_csv(f'{args.out_dir}/cluster_sizes.tsv', sep='\t')
    return result


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
