"""Drop-in for the reference ``interpret_features.py`` and ``interpret_features_grouped.py`` CLIs:
Ward clustering of the expression model's features (or, ``--grouped``, of the chromatin marks) over
the training genes.  It writes the ``all_feature_clusters.tsv`` that
``expecto_amd.predict_by_cluster --feature_clusters_df`` reads.

    python -m expecto_amd.interpret_features --belugaFeatures features.tsv --targetIndex 1 \\
        --expFile geneanno.exp.csv --inputFile Xreducedall.2002.npy --annoFile geneanno.csv \\
        [--grouped] [--n_clusters K] [--clustering_joblib out/clustering.npz] --out_dir out

Arguments are those of ``interpret_features.py:17-36`` plus ``--grouped`` and ``--n_clusters``
(the reference hard-codes 10, and 110 in the grouped script).  The gene filter, the train split and
the ``Cell type:`` line are the reference's (``interpret_features.py:45-74``).

The reference fits sklearn's ``AgglomerativeClustering``, whose unstructured Ward path is scipy's
``pdist`` followed by its NN-chain linkage.  Here the distance matrix is one device kernel
(``expecto_pairwise_euclidean``: float64, scipy's summation order, so scipy's bits) and the linkage
is host C++ (``expecto_ward_linkage``); the tree, and with it every label, equals sklearn's.

* ungrouped: the points are the ``10 x marks`` features, ``X_train.T``; outputs of
  ``interpret_features.py:116-134``: ``all_feature_clusters.tsv`` (ten rows per mark, columns
  ``coeff_idx`` and ``cluster``) and ``clusters/cluster_i.tsv``.
* ``--grouped``: the points are the marks, each with its ten exp-decay features of every training
  gene (:func:`features_grouped`); outputs of ``interpret_features_grouped.py:143-162``, which add
  ``cluster_sizes.tsv``.

The mark count is that of the ``--belugaFeatures`` table; ``--inputFile`` must have ten columns
per mark.  The tree is saved as ``<out_dir>/clustering.npz`` (``children``, ``distances``,
``n_leaves``); ``--clustering_joblib`` takes that file and cuts it again without a device, or a
sklearn ``.joblib`` dump where joblib and sklearn are installed.  ``--clustering_with_distances`` is
accepted: distances are always kept.  The silhouette sweep and the dendrogram the reference has
commented out are left out.
"""
from __future__ import annotations

import argparse
import ctypes
import heapq
import os
import sys

import numpy as np
import pandas as pd

N_CLUSTERS = 10             # interpret_features.py:116
N_CLUSTERS_GROUPED = 108 + 2  # interpret_features_grouped.py:143


def build_parser():
    parser = argparse.ArgumentParser(description='Ward clustering of ExPecto features or chromatin marks.')
    parser.add_argument('--clustering_joblib', action='store', dest='clustering_joblib', type=str, default=None,
                        help="clustering.npz of an earlier run (or a sklearn joblib dump). If None, recomputes the "
                             "hierarchical clustering given the inputFile training data.")
    parser.add_argument('--clustering_with_distances', action="store_true", default=False)
    parser.add_argument('--belugaFeatures', action="store", dest="belugaFeatures",
                        help="tsv file denoting Beluga features")
    parser.add_argument('--targetIndex', action="store", dest="targetIndex", type=int)
    parser.add_argument('--expFile', action="store", dest="expFile")
    parser.add_argument('--inputFile', action="store", dest="inputFile", default='./resources/Xreducedall.2002.npy')
    parser.add_argument('--annoFile', action="store", dest="annoFile", default='./resources/geneanno.csv')
    parser.add_argument('--filterStr', action="store", dest="filterStr", type=str, default="all")
    parser.add_argument('--pseudocount', action="store", dest="pseudocount", type=float, default=0.0001)
    parser.add_argument('--out_dir', type=str, default='interpret_features')
    parser.add_argument('--grouped', action="store_true", default=False,
                        help="cluster the marks (interpret_features_grouped.py) instead of the 10 x marks features")
    parser.add_argument('--n_clusters', type=int, default=None,
                        help=f"clusters to cut the tree into (default {N_CLUSTERS}, grouped {N_CLUSTERS_GROUPED})")
    return parser


def features_grouped(X_train, n_marks: int):
    """[genes, 10 * n_marks] -> [n_marks, genes * 10]: point f, dimension g*10 + k is
    ``X_train[g, k*n_marks + f]`` (interpret_features_grouped.py:73).  numpy in, numpy out; a torch
    tensor gives a (strided) torch view on its device."""
    if X_train.ndim != 2 or X_train.shape[1] != 10 * n_marks:
        raise ValueError(f"features_grouped: expected [genes, {10 * n_marks}] for {n_marks} marks, "
                         f"got {tuple(X_train.shape)}")
    g = X_train.shape[0]
    if isinstance(X_train, np.ndarray):
        return X_train.reshape(g, 10, n_marks).transpose(2, 0, 1).reshape(n_marks, g * 10)
    return X_train.reshape(g, 10, n_marks).permute(2, 0, 1).reshape(n_marks, g * 10)


def ward_tree(X, device=None):
    """Ward tree of the rows of ``X`` ([n_points, n_dims], numpy array or torch tensor): ``(children
    [int64, n-1, 2], distances [float64, n-1])``, equal to ``AgglomerativeClustering(...).fit(X)``'s
    ``children_`` and ``distances_``.  The distances are computed on ``device`` (default: the current
    HIP device), the condensed matrix (``8 * n(n-1)/2`` bytes) is copied to the host and linked
    there.  ValueError on fewer than 2 points or a NaN / infinity in ``X``."""
    import torch

    from . import _lib

    if isinstance(X, np.ndarray) and not X.flags.writeable:
        X = X.copy()     # torch does not wrap read-only arrays
    t = torch.from_numpy(X) if isinstance(X, np.ndarray) else X
    if t.dim() != 2:
        raise ValueError(f"ward_tree: expected a 2-D array of points, got shape {tuple(t.shape)}")
    n, d = int(t.shape[0]), int(t.shape[1])
    if n < 2:
        raise ValueError(f"ward_tree: found {n} point(s), at least 2 are required")
    if not bool(torch.isfinite(t).all()):
        raise ValueError("ward_tree: input X contains NaN or infinity")
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        x = t.to(device=dev, dtype=torch.float64).contiguous()
        cond = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device=dev)
        _lib.check(lib.expecto_pairwise_euclidean(_lib.dptr(x), n, d, max(d, x.stride(0)), _lib.dptr(cond),
                                                  _lib.stream_ptr()), "expecto_pairwise_euclidean")
        cond = cond.cpu().numpy()
    return _link(lib, cond, n)


def _link(lib, cond: np.ndarray, n: int):
    children = np.empty((n - 1, 2), np.int32)
    heights = np.empty(n - 1, np.float64)
    sizes = np.empty(n - 1, np.int32)
    st = lib.expecto_ward_linkage(cond.ctypes.data_as(ctypes.c_void_p), n, children.ctypes.data_as(ctypes.c_void_p),
                                  heights.ctypes.data_as(ctypes.c_void_p), sizes.ctypes.data_as(ctypes.c_void_p))
    if st != 0:
        raise ValueError(lib.expecto_last_error().decode())
    return children.astype(np.int64), heights


def cut_tree(children, n_leaves: int, n_clusters: int):
    """Labels [int64, n_leaves] of the tree cut into ``n_clusters``: sklearn's ``_hc_cut``, with its
    label numbering (label i is the i-th entry of the heap list in its stored order)."""
    children = np.asarray(children)
    if children.shape != (n_leaves - 1, 2):
        raise ValueError(f"cut_tree: children of shape {children.shape} for {n_leaves} leaves")
    if not 1 <= n_clusters <= n_leaves:
        raise ValueError(f"Cannot extract more clusters than samples: {n_clusters} clusters were given for a tree "
                         f"with {n_leaves} leaves.")
    nodes = [-(int(max(children[-1])) + 1)]
    for _ in range(n_clusters - 1):
        these_children = children[-nodes[0] - n_leaves]
        heapq.heappush(nodes, -int(these_children[0]))
        heapq.heappushpop(nodes, -int(these_children[1]))
    label = np.zeros(n_leaves, dtype=np.int64)
    for i, node in enumerate(nodes):
        stack = [-node]
        while stack:
            v = stack.pop()
            if v < n_leaves:
                label[v] = i
            else:
                stack.extend(int(c) for c in children[v - n_leaves])
    return label


def load_tree(path: str):
    """(children, distances or None, n_leaves) from a clustering.npz, or from a sklearn joblib dump."""
    if path.endswith(".npz"):
        z = np.load(path)
        return z["children"].astype(np.int64), z["distances"], int(z["n_leaves"])
    try:
        import joblib
        import sklearn  # noqa: F401  -- the dump unpickles into its classes
    except ImportError as e:
        raise RuntimeError(f"--clustering_joblib {path}: reading a sklearn joblib dump needs joblib and scikit-learn "
                           f"({e}); pass the clustering.npz this program writes instead") from e
    model = joblib.load(path)
    return (np.asarray(model.children_, np.int64), getattr(model, "distances_", None), int(model.n_leaves_))


def training_rows(args) -> np.ndarray:
    """interpret_features.py:45-70: the feature rows of the training genes."""
    Xreducedall = np.load(args.inputFile)
    geneanno = pd.read_csv(args.annoFile)

    if args.filterStr == 'pc':
        filt = np.asarray(geneanno.iloc[:, -1] == 'protein_coding')
    elif args.filterStr == 'lincRNA':
        filt = np.asarray(geneanno.iloc[:, -1] == 'lincRNA')
    elif args.filterStr == 'all':
        filt = np.asarray(geneanno.iloc[:, -1] != 'rRNA')
    else:
        raise ValueError('filterStr has to be one of all, pc, and lincRNA')

    geneexp = pd.read_csv(args.expFile)
    print(f"Cell type: {geneexp.columns[args.targetIndex]}")

    with np.errstate(divide="ignore", invalid="ignore"):
        filt = filt * np.isfinite(np.asarray(np.log(geneexp.iloc[:, args.targetIndex] + args.pseudocount)))

    trainind = np.asarray(geneanno['seqnames'] != 'chrX') * np.asarray(geneanno['seqnames'] != 'chrY') \
        * np.asarray(geneanno['seqnames'] != 'chr8')
    return Xreducedall[trainind * filt, :]


def run(args):
    from . import predict

    os.makedirs(args.out_dir, exist_ok=True)
    X_train = training_rows(args)
    beluga_features_df = predict.read_features_table(args.belugaFeatures)
    n_marks = beluga_features_df.shape[0]
    if X_train.shape[1] != 10 * n_marks:
        raise ValueError(f"--inputFile has {X_train.shape[1]} columns, --belugaFeatures lists {n_marks} marks "
                         f"(10 columns per mark: {10 * n_marks})")
    n_points = n_marks if args.grouped else 10 * n_marks
    n_clusters = args.n_clusters if args.n_clusters is not None else (N_CLUSTERS_GROUPED if args.grouped
                                                                      else N_CLUSTERS)

    if args.clustering_joblib is None:
        print("Clustering and saving model to joblib..." if args.clustering_with_distances
              else "Clustering complete tree and caching...")
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("expecto_amd.interpret_features needs a GPU (HIP) to cluster; there is no CPU path")
        x = torch.from_numpy(X_train).cuda()
        children, distances = ward_tree(features_grouped(x, n_marks) if args.grouped else x.T)
        np.savez(f'{args.out_dir}/clustering.npz', children=children, distances=distances, n_leaves=n_points)
    else:
        print(f"Loading clustering model from {args.clustering_joblib}...")
        children, distances, n_leaves = load_tree(args.clustering_joblib)
        if n_leaves != n_points:
            raise ValueError(f"{args.clustering_joblib} holds a tree of {n_leaves} leaves, this run clusters "
                             f"{n_points} points")

    clusters = cut_tree(children, n_points, n_clusters)

    # Save clusters to file
    if args.grouped:
        input_features_df = beluga_features_df
        input_features_df['cluster'] = clusters.ravel()
    else:
        clusters = clusters.reshape(10, n_marks).transpose(1, 0)
        input_features_df = pd.DataFrame(np.repeat(beluga_features_df.values, 10, axis=0))
        input_features_df.columns = beluga_features_df.columns
        input_features_df['coeff_idx'] = np.tile(np.arange(10), beluga_features_df.shape[0])
        input_features_df['cluster'] = clusters.ravel()
    input_features_df.to_csv(f'{args.out_dir}/all_feature_clusters.tsv', sep='\t')

    cluster_dir = f'{args.out_dir}/clusters'
    os.makedirs(cluster_dir, exist_ok=True)
    sizes_df = pd.DataFrame(columns=['size'])
    for i in range(n_clusters):
        cluster_df = input_features_df[input_features_df['cluster'] == i]
        cluster_df.to_csv(f'{cluster_dir}/cluster_{i}.tsv', sep='\t')
        sizes_df.loc[f'cluster_{i}'] = cluster_df.shape[0]

    if args.grouped:
        sizes_df = sizes_df.sort_values(by='size', ascending=False)
        sizes_df.to_csv(f'{args.out_dir}/cluster_sizes.tsv', sep='\t')
    return children, distances, clusters


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
