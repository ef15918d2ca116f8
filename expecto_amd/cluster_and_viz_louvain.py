"""Drop-in for the reference ``cluster_and_viz_louvain.py``: Louvain communities of the marks' SVD
coordinates (``tf_idf_reduced_100.npy`` of ``expecto_amd.svd``) on the GPU, and the cluster files that
``predict_by_cluster --feature_clusters_df`` reads.  Unlike Ward and k-means, the number of clusters comes
from the data.

    python -m expecto_amd.cluster_and_viz_louvain <svd_transform_dir> --belugaFeatures features.tsv [ablation flags] \\
        [-o temp_cluster_and_viz] [--n_pcs 20] [--k_neighbors 5] [--resolution 1.0] [--seed 0] [--n_init 1] \\
        [--resolution_sweep G_MIN G_MAX STEP] [--tsne] [--tsne_perplexity 30] [--tsne_iter 1000] [--tsne_init pca|random]

The reference runs Orange's ``Louvain(5)`` on the first 20 coordinates: a 5-nearest-neighbour graph with
Jaccard edge weights, then python-louvain.  Neither package was available, so the algorithm is defined in
include/expecto_hip.h from the published definitions (Blondel et al. 2008; the resolution of Reichardt and
Bornholdt) and anchored by the tests to scikit-learn's ``NearestNeighbors`` and to networkx's
``modularity``; how closely its partitions agree with Orange's is unmeasured.  The graph
(``expecto_knn_jaccard``) and the search (``expecto_louvain``) run on the device in float64 with a fixed
order of every sum; symmetrising the neighbour lists into CSR is numpy on the host.  A Louvain result
depends on the resolution and on the order in which nodes are visited, so ``--resolution_sweep`` and
``--n_init`` run every (resolution, restart) as one problem of a single launch; restart r visits the nodes
in ``np.random.RandomState(seed + r).permutation(n)``, and the restart of largest modularity is kept, the
first on ties.

Files: ``all_feature_clusters.tsv``, ``clusters/cluster_<i>.tsv`` and ``cluster_sizes.tsv`` in
``cluster_and_viz``'s layout; ``louvain.json``; with the sweep ``resolution_sweep.tsv`` (the cluster files
stay those of ``--resolution``); with ``--tsne`` the files of ``cluster_and_viz.write_tsne``.  Nothing is
shown; a picture is saved only where matplotlib imports.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import NamedTuple

import numpy as np

from . import cluster_and_viz

N_PCS = 20          # cluster_and_viz_louvain.py:48
K_NEIGHBORS = 5     # cluster_and_viz_louvain.py:52
MAX_N, MAX_D, MAX_K = 4096, 128, 64     # include/expecto_hip.h
PASS_BOUND, LEVEL_BOUND, BAD_GRAPH = 1, 2, 4


class LouvainResult(NamedTuple):
    labels: np.ndarray        # int32 [n], communities numbered by their smallest member
    modularity: float
    n_communities: int
    n_levels: int             # levels aggregated
    n_passes: int             # local-moving passes of all levels
    restart: int              # the winning restart: the first of maximal modularity
    flags: int                # PASS_BOUND | LEVEL_BOUND: a bound ended a loop before its stop


def _checked(X, k_neighbors):
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if X.ndim != 2:
        raise ValueError(f"louvain: X must be 2-D, got shape {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError("louvain: X contains NaN or infinity")
    n, d = X.shape
    if not (1 <= n <= MAX_N and 1 <= d <= MAX_D):
        raise ValueError(f"louvain: X has shape {X.shape}; supported are 1..{MAX_N} points of 1..{MAX_D} dimensions")
    k = int(k_neighbors)
    if not 1 <= k <= min(n, MAX_K):
        raise ValueError(f"louvain: k_neighbors = {k} outside [1, min(n, {MAX_K})] with n = {n}")
    return X, k


def knn_graph(X, k_neighbors=K_NEIGHBORS, device=None, timings=None):
    """``expecto_knn_jaccard`` of X: (nbr int32 [n, k], w float64 [n, k]) as host arrays.  ``nbr[i]`` is
    ``NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)[1][i]`` with ties to the lower index; ``w`` the
    Jaccard index of the two neighbour sets, 0 where a point is its own neighbour."""
    X, k = _checked(X, k_neighbors)
    from . import _lib
    torch = _lib.require_gpu("cluster_and_viz_louvain")
    dev = _lib.device_of(device)
    n, d = X.shape
    with torch.cuda.device(dev):
        Xd = _lib.upload(X, dev)
        nbr = torch.empty((n, k), dtype=torch.int32, device=dev)
        w = torch.empty((n, k), dtype=torch.float64, device=dev)
        timer = _lib.EventTimer(timings)
        timer.mark()
        _lib.call("expecto_knn_jaccard", Xd.data_ptr(), n, d, d, k, nbr.data_ptr(), w.data_ptr())
        timer.mark(sync=True)
        timer.set("graph_ms")
        return nbr.cpu().numpy(), w.cpu().numpy()


def symmetrize(nbr, w):
    """The undirected graph of the neighbour lists as CSR (indptr int32 [n + 1], indices int32, weights
    float64): an edge {i, j}, i != j, where j is in N(i) or i in N(j), its weight the Jaccard value (the
    same from either side), no self-loops, rows ascending in neighbour index."""
    nbr, w = np.asarray(nbr), np.asarray(w, np.float64)
    n, k = nbr.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = nbr.astype(np.int64).ravel()
    keep = rows != cols
    rows, cols, vals = rows[keep], cols[keep], w.ravel()[keep]
    key = np.concatenate([rows * n + cols, cols * n + rows])
    key, first = np.unique(key, return_index=True)
    weights = np.concatenate([vals, vals])[first]
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(key // n, minlength=n), out=indptr[1:])
    return indptr, (key % n).astype(np.int32), np.ascontiguousarray(weights)


def run_problems(indptr, indices, weights, gammas, perms, max_passes=100, max_levels=32, device=None, timings=None):
    """``expecto_louvain`` of the CSR graph for the problems ``(gammas[p], perms[p])`` in one launch.
    Returns per problem ``(labels, modularity, n_communities, n_levels, n_passes, flags)``.  ``timings``
    receives the launch's device ms (``louvain_ms``)."""
    from . import _lib
    torch = _lib.require_gpu("cluster_and_viz_louvain")
    dev = _lib.device_of(device)
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    weights = np.ascontiguousarray(weights, np.float64)
    gammas = np.ascontiguousarray(gammas, np.float64)
    perms = np.ascontiguousarray(perms, np.int32)
    n, nnz, P = indptr.size - 1, indices.size, gammas.size
    if perms.shape != (P, n):
        raise ValueError(f"louvain: perms has shape {perms.shape}, expected {(P, n)}")
    if not np.isfinite(gammas).all():
        raise ValueError("louvain: a resolution is NaN or infinite")
    if P == 0:
        return []
    nbytes = int(_lib.load().expecto_louvain_workspace(n, nnz, P))
    with torch.cuda.device(dev):
        d_ptr, d_idx, d_w, d_g, d_perm = (_lib.upload(a, dev) for a in (indptr, indices, weights, gammas, perms))
        labels = torch.empty((P, n), dtype=torch.int32, device=dev)
        modularity = torch.empty(P, dtype=torch.float64, device=dev)
        counters = torch.empty((P, 4), dtype=torch.int32, device=dev)
        ws = _lib.workspace(nbytes + 8, dev)
        timer = _lib.EventTimer(timings)
        timer.mark()
        _lib.call("expecto_louvain", d_ptr.data_ptr(), d_idx.data_ptr(), d_w.data_ptr(), n, nnz, P,
                  d_g.data_ptr(), d_perm.data_ptr(), int(max_passes), int(max_levels), labels.data_ptr(),
                  modularity.data_ptr(), counters.data_ptr(), ws.data_ptr(), nbytes)
        timer.mark(sync=True)
        timer.set("louvain_ms")
        labels, modularity, counters = labels.cpu().numpy(), modularity.cpu().numpy(), counters.cpu().numpy()
    if (counters[:, 3] & BAD_GRAPH).any():
        raise ValueError("louvain: the graph is not a CSR matrix over n nodes, or an order is not a permutation")
    return [(labels[p], float(modularity[p]), int(counters[p, 0]), int(counters[p, 1]), int(counters[p, 2]),
             int(counters[p, 3])) for p in range(P)]


def permutation(seed, restart, n):
    """The order in which restart ``restart`` visits the nodes at level 0."""
    return np.random.RandomState(int(seed) + int(restart)).permutation(n).astype(np.int32)


def louvain_sweep(X, k_neighbors=K_NEIGHBORS, resolutions=(1.0,), n_init=1, seed=0, max_passes=100, max_levels=32,
                  device=None, timings=None):
    """Louvain communities of X's ``k_neighbors``-nearest-neighbour Jaccard graph for every resolution of
    ``resolutions``: all ``len(resolutions) * n_init`` problems in one launch.  Returns one
    :class:`LouvainResult` per resolution, of the restart of maximal modularity (the first on ties).
    ``timings``: a dict that receives ``graph_ms`` and ``louvain_ms`` (device, events) and ``symmetrize_ms``
    (host)."""
    import time

    X, k = _checked(X, k_neighbors)
    n_init = int(n_init)
    if n_init < 1:
        raise ValueError("louvain: n_init must be at least 1")
    resolutions = [float(g) for g in resolutions]
    n = X.shape[0]
    nbr, w = knn_graph(X, k, device=device, timings=timings)
    t0 = time.perf_counter()
    indptr, indices, weights = symmetrize(nbr, w)
    if timings is not None:
        timings["symmetrize_ms"] = (time.perf_counter() - t0) * 1e3
    perms = np.stack([permutation(seed, r, n) for r in range(n_init)])
    res = run_problems(indptr, indices, weights, np.repeat(resolutions, n_init), np.tile(perms, (len(resolutions), 1)),
                       max_passes=max_passes, max_levels=max_levels, device=device, timings=timings)
    out = []
    for i in range(len(resolutions)):
        per = res[i * n_init:(i + 1) * n_init]
        r = int(np.argmax([p[1] for p in per]))       # the first of maximal modularity
        out.append(LouvainResult(per[r][0], per[r][1], per[r][2], per[r][3], per[r][4], r, per[r][5]))
    return out


def louvain(X, k_neighbors=K_NEIGHBORS, resolution=1.0, n_init=1, seed=0, max_passes=100, max_levels=32,
            device=None) -> LouvainResult:
    """:func:`louvain_sweep` of a single resolution."""
    return louvain_sweep(X, k_neighbors, [resolution], n_init=n_init, seed=seed, max_passes=max_passes,
                         max_levels=max_levels, device=device)[0]


# ---- CLI -------------------------------------------------------------------------------------

def build_parser():
    """``cluster_and_viz``'s arguments without the k-means ones, and the knobs the reference has as
    constants (cluster_and_viz_louvain.py:48,52)."""
    parser = argparse.ArgumentParser(prog="python -m expecto_amd.cluster_and_viz_louvain",
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
    parser.add_argument('--k_neighbors', type=int, default=K_NEIGHBORS, help='neighbours per mark in the graph')
    parser.add_argument('--resolution', type=float, default=1.0, help='above 1: more, smaller clusters')
    parser.add_argument('--seed', type=int, default=0, help='restart r visits the marks in RandomState(seed + r) order')
    parser.add_argument('--n_init', type=int, default=1, help='restarts; the best modularity is kept')
    parser.add_argument('--resolution_sweep', type=float, nargs=3, metavar=('G_MIN', 'G_MAX', 'STEP'), default=None,
                        help='also run every resolution of arange(G_MIN, G_MAX, STEP) and write resolution_sweep.tsv')
    parser.add_argument('--tsne', action='store_true', default=False,
                        help='also embed the marks in two dimensions (exact t-SNE): tsne_embedding.tsv, tsne.json, tsne.png')
    parser.add_argument('--tsne_perplexity', type=float, default=30.0)
    parser.add_argument('--tsne_iter', type=int, default=1000, help='iterations of the t-SNE descent at most')
    parser.add_argument('--tsne_init', choices=('pca', 'random'), default='pca')
    return parser


def sweep_resolutions(g_min, g_max, step):
    """``g_min + i * step`` for i = 0, 1, ... below ``g_max``, each rounded to 10 decimals."""
    if not (step > 0 and g_max > g_min and (g_max - g_min) / step <= 10000):
        raise ValueError(f"--resolution_sweep {g_min} {g_max} {step}: an empty or endless range")
    out, i = [], 0
    while round(g_min + i * step, 10) < g_max:
        out.append(round(g_min + i * step, 10))
        i += 1
    return out


def write_clusters(out_dir, input_features_df, k):
    """``clusters/cluster_<i>.tsv`` and ``cluster_sizes.tsv`` of a table with a ``cluster`` column, as
    ``cluster_and_viz.run`` writes them (cluster_and_viz.py:69-103)."""
    import pandas as pd

    input_features_df.to_csv(f'{out_dir}/all_feature_clusters.tsv', sep='\t')
    cluster_dir = f'{out_dir}/clusters'
    os.makedirs(cluster_dir, exist_ok=True)
    sizes_df = pd.DataFrame(columns=['size'])
    for i in range(k):
        cluster_df = input_features_df[input_features_df['cluster'] == i]
        cluster_df.to_csv(f'{cluster_dir}/cluster_{i}.tsv', sep='\t')
        sizes_df.loc[f'cluster_{i}'] = cluster_df.shape[0]
    sizes_df = sizes_df.sort_values(by='size', ascending=False)
    sizes_df.to_csv(f'{out_dir}/cluster_sizes.tsv', sep='\t')


def summary(result, args):
    """The contents of ``louvain.json``."""
    return {'modularity': result.modularity, 'n_clusters': result.n_communities, 'n_levels': result.n_levels,
            'n_passes': result.n_passes, 'resolution': args.resolution, 'k_neighbors': args.k_neighbors,
            'seed': args.seed, 'restart': result.restart, 'flags': result.flags}


def run(args):
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

    if args.resolution_sweep is not None:
        gs = sweep_resolutions(*args.resolution_sweep)
        swept = louvain_sweep(X, args.k_neighbors, gs, n_init=args.n_init, seed=args.seed)
        with open(f'{args.out_dir}/resolution_sweep.tsv', 'w') as f:
            f.write('resolution\tn_clusters\tmodularity\trestart\n')
            f.writelines(f'{g!r}\t{r.n_communities}\t{r.modularity!r}\t{r.restart}\n' for g, r in zip(gs, swept))

    result = louvain(X, args.k_neighbors, args.resolution, n_init=args.n_init, seed=args.seed)
    labels, k = result.labels, result.n_communities

    input_features_df = beluga_features_df[keep_mask].copy()
    input_features_df['cluster'] = labels
    write_clusters(args.out_dir, input_features_df, k)
    with open(f'{args.out_dir}/louvain.json', 'w') as f:
        json.dump(summary(result, args), f, indent=1)
        f.write('\n')
    if args.tsne:
        cluster_and_viz.write_tsne(args, X, input_features_df, labels, k)
    return result


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
