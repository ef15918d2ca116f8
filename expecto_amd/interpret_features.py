"""Drop-in for the reference ``interpret_features.py`` and ``interpret_features_grouped.py`` CLIs:
Ward clustering of the expression model's features (or, ``--grouped``, of the chromatin marks) over
the training genes.  It writes the ``all_feature_clusters.tsv`` that
``expecto_amd.predict_by_cluster --feature_clusters_df`` reads.

    python -m expecto_amd.interpret_features --belugaFeatures features.tsv --targetIndex 1 \\
        --expFile geneanno.exp.csv --inputFile Xreducedall.2002.npy --annoFile geneanno.csv \\
        [--grouped] [--n_clusters K|auto] [--silhouette K_MIN K_MAX] \\
        [--clustering_joblib out/clustering.npz] --out_dir out

Arguments are those of ``interpret_features.py:17-36`` plus ``--grouped``, ``--n_clusters`` (the
reference hard-codes 10, and 110 in the grouped script) and ``--silhouette``.  The gene filter, the
train split and the ``Cell type:`` line are the reference's (``interpret_features.py:45-74``).

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
accepted: distances are always kept.  The dendrogram the reference has commented out is left out.

``--silhouette K_MIN K_MAX`` is the sweep of ``interpret_features_grouped.py:120-144`` that chose the
reference's 110: the silhouette score of the tree cut into every ``k`` of the inclusive range
(``K_MAX`` clipped to ``n_points - 1``), written to ``<out_dir>/silhouette_scores.tsv``, and
``--n_clusters auto`` cuts at its first maximum.  The cuts of one tree are nested, so one pass over
the distance matrix serves every ``k`` (:func:`silhouette_sweep`): the per-point distance sums of the
``K_MIN + 2 (K_MAX - K_MIN)`` tree nodes that some cut uses, then the samples of every cut, both on
the device from the exact ``pdist`` distances.  The samples equal
``sklearn.metrics.silhouette_samples(squareform(pdist(X)), labels, metric='precomputed')`` bit for
bit (include/expecto_hip.h states the arithmetic).  With ``--clustering_joblib`` the tree is loaded
and only the distances are recomputed.  The reference's PNG of the scores is left out.
"""
from __future__ import annotations

import argparse
import heapq
import operator
import os
import sys
from typing import NamedTuple

import numpy as np
import pandas as pd

N_CLUSTERS = 10             # interpret_features.py:116
N_CLUSTERS_GROUPED = 108 + 2  # interpret_features_grouped.py:143


def n_clusters_arg(text: str):
    """--n_clusters: an integer, or 'auto'."""
    return text if text == 'auto' else int(text)


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
    parser.add_argument('--n_clusters', type=n_clusters_arg, default=None,
                        help=f"clusters to cut the tree into (default {N_CLUSTERS}, grouped {N_CLUSTERS_GROUPED}); "
                             f"'auto' (with --silhouette): the first maximum of the silhouette score")
    parser.add_argument('--silhouette', type=int, nargs=2, metavar=('K_MIN', 'K_MAX'), default=None,
                        help="write the silhouette score of every cut from K_MIN to K_MAX clusters (inclusive; K_MAX "
                             "is clipped to n_points - 1) to <out_dir>/silhouette_scores.tsv")
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


def pairwise_condensed(X, device=None, what="pairwise_condensed"):
    """scipy's ``pdist(X)`` (float64, its bits) of the rows of ``X`` ([n_points, n_dims], numpy array
    or torch tensor) as a tensor on ``device`` (default: the current HIP device).  ValueError on fewer
    than 2 points or a NaN / infinity in ``X``."""
    import torch

    from . import _lib

    if isinstance(X, np.ndarray) and not X.flags.writeable:
        X = X.copy()     # torch does not wrap read-only arrays
    t = torch.from_numpy(X) if isinstance(X, np.ndarray) else X
    if t.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D array of points, got shape {tuple(t.shape)}")
    n, d = int(t.shape[0]), int(t.shape[1])
    if n < 2:
        raise ValueError(f"{what}: found {n} point(s), at least 2 are required")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: input X contains NaN or infinity")
    dev = _lib.device_of(device)
    with torch.cuda.device(dev):
        x = t.to(device=dev, dtype=torch.float64).contiguous()
        cond = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device=dev)
        _lib.call("expecto_pairwise_euclidean", _lib.dptr(x), n, d, max(d, x.stride(0)), _lib.dptr(cond))
    return cond


def ward_tree(X, device=None, return_condensed=False):
    """Ward tree of the rows of ``X`` ([n_points, n_dims], numpy array or torch tensor): ``(children
    [int64, n-1, 2], distances [float64, n-1])``, equal to ``AgglomerativeClustering(...).fit(X)``'s
    ``children_`` and ``distances_``.  The distances are computed on ``device`` (default: the current
    HIP device), the condensed matrix (``8 * n(n-1)/2`` bytes) is copied to the host and linked
    there.  ValueError on fewer than 2 points or a NaN / infinity in ``X``.  With
    ``return_condensed`` the device tensor of the distances (:func:`pairwise_condensed`) is returned
    as a third value; the linkage overwrites its host copy only."""
    cond = pairwise_condensed(X, device, "ward_tree")
    n = int(X.shape[0])
    children, heights = _link(cond.cpu().numpy(), n)
    return (children, heights, cond) if return_condensed else (children, heights)


def _link(cond: np.ndarray, n: int):
    from . import _lib

    children = np.empty((n - 1, 2), np.int32)
    heights = np.empty(n - 1, np.float64)
    sizes = np.empty(n - 1, np.int32)
    _lib.host_call("expecto_ward_linkage", cond.ctypes.data, n, children.ctypes.data, heights.ctypes.data,
                   sizes.ctypes.data, prefix=False)
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


# ---- silhouette of the tree's cuts ----------------------------------------------------------------

class SweepPlan(NamedTuple):
    """What the two silhouette kernels read (include/expecto_hip.h).  ``nodes``: ids of the tree
    nodes some cut uses, ascending; row v of the node sums belongs to ``nodes[v]``."""
    nodes: np.ndarray      # int64 [n_nodes]
    node_ptr: np.ndarray   # int64 [n_nodes + 1]: members[node_ptr[v]:node_ptr[v+1]] are row v's points, ascending
    members: np.ndarray    # int32
    sizes: np.ndarray      # int32 [n_nodes]
    cut_ptr: np.ndarray    # int64 [n_cuts + 1]: active[cut_ptr[c]:cut_ptr[c+1]] are the rows of cut c
    active: np.ndarray     # int32
    own: np.ndarray        # int32 [n_cuts, n]: the row of cut c that holds point i


def _checked_ks(ks, n: int):
    ks = [operator.index(k) for k in ks]
    for k in ks:
        if not 2 <= k <= n - 1:
            raise ValueError(f"silhouette: n_clusters is {k}. Valid values are 2 to n_samples - 1 = {n - 1} "
                             f"(inclusive)")
    if len(set(ks)) != len(ks):
        raise ValueError(f"silhouette: duplicate n_clusters among {ks}")
    return ks


def plan_sweep(children, n_leaves: int, ks) -> SweepPlan:
    """Host plan of a silhouette sweep over the cuts ``ks`` (any distinct values of 2..n-1, in any
    order) of the tree ``children``.  Merge m made node n + m, so ids ascend with the height and
    ``cut_tree`` splits the largest id first: the clusters of cut k are the nodes below 2n - k whose
    parent is not.  Going from k to k + 1 replaces one node by its two children, so a contiguous sweep
    needs ``k_min + 2 (k_max - k_min)`` nodes."""
    n = int(n_leaves)
    children = np.asarray(children)
    if n < 3 or children.shape != (n - 1, 2):
        raise ValueError(f"plan_sweep: children of shape {children.shape} for {n} leaves (at least 3)")
    ks = _checked_ks(ks, n)
    ch = children.astype(np.int64)
    made = n + np.arange(n - 1)
    if ch.min() < 0 or (ch >= made[:, None]).any() or (np.bincount(ch.ravel(), minlength=2 * n - 1)[:2 * n - 2] != 1).any():
        raise ValueError("plan_sweep: children is not a merge tree (a child made after its parent, or joined twice)")
    parent = np.full(2 * n - 1, 2 * n - 1, np.int64)
    parent[ch[:, 0]] = made
    parent[ch[:, 1]] = made
    size = np.ones(2 * n - 1, np.int64)
    for m in range(n - 1):
        size[n + m] = size[ch[m, 0]] + size[ch[m, 1]]
    start = np.zeros(2 * n - 1, np.int64)      # every node is a range of the leaves in dendrogram order
    for v in range(2 * n - 2, n - 1, -1):
        a, b = ch[v - n]
        start[a] = start[v]
        start[b] = start[v] + size[a]
    order = np.empty(n, np.int64)
    order[start[:n]] = np.arange(n)

    ids = np.arange(2 * n - 1)
    need = np.zeros(2 * n - 1, bool)
    for k in ks:
        need |= (ids < 2 * n - k) & (parent >= 2 * n - k)
    nodes = np.nonzero(need)[0]
    sizes = size[nodes]
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    members = np.empty(node_ptr[-1], np.int32)
    for v, node in enumerate(nodes):
        members[node_ptr[v]:node_ptr[v + 1]] = np.sort(order[start[node]:start[node] + size[node]])

    cut_ptr = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    active = np.empty(cut_ptr[-1], np.int32)
    own = np.empty((len(ks), n), np.int32)
    for c, k in enumerate(ks):
        rows = np.nonzero(parent[nodes[nodes < 2 * n - k]] >= 2 * n - k)[0]    # nodes ascends: rows index it
        rows = rows[np.argsort(start[nodes[rows]], kind="stable")]           # in dendrogram order they tile 0..n
        active[cut_ptr[c]:cut_ptr[c + 1]] = rows
        own[c, order] = np.repeat(rows, sizes[rows])
    return SweepPlan(nodes, node_ptr, members, sizes.astype(np.int32), cut_ptr, active, own)


def _device_condensed(condensed, n: int):
    """The n(n-1)/2 distances as a float64 device tensor; ValueError on a wrong length or a NaN /
    infinity (a numpy array is checked on the host, before any device call)."""
    import torch

    if isinstance(condensed, np.ndarray):
        if condensed.shape != (n * (n - 1) // 2,):
            raise ValueError(f"silhouette: {n} points have {n * (n - 1) // 2} distances, got shape {condensed.shape}")
        if not np.isfinite(condensed).all():
            raise ValueError("silhouette: the distance matrix contains NaN or infinity")
        return torch.from_numpy(np.ascontiguousarray(condensed, np.float64)).cuda()
    if tuple(condensed.shape) != (n * (n - 1) // 2,):
        raise ValueError(f"silhouette: {n} points have {n * (n - 1) // 2} distances, got shape {tuple(condensed.shape)}")
    from . import _lib
    _lib.dptr(condensed)    # a device tensor, or RuntimeError
    if not bool(torch.isfinite(condensed).all()):
        raise ValueError("silhouette: the distance matrix contains NaN or infinity")
    return condensed.to(torch.float64).contiguous()


def _run_plan(cond, n: int, plan: SweepPlan) -> np.ndarray:
    """samples float64 [n_cuts, n] of the plan's cuts: node sums, then cuts, on the device of ``cond``.
    The distances are expanded to the square matrix where it fits beside the rest; the condensed
    matrix is indexed directly otherwise (same bits)."""
    import torch

    from . import _lib

    dev = cond.device
    n_nodes, n_cuts = len(plan.sizes), len(plan.cut_ptr) - 1
    with torch.cuda.device(dev):
        s_bytes, out_bytes = 8 * n_nodes * n, 8 * n_cuts * n
        lists = 4 * n_cuts * n + plan.members.nbytes + plan.active.nbytes + plan.node_ptr.nbytes + plan.cut_ptr.nbytes \
            + plan.sizes.nbytes
        need = s_bytes + out_bytes + lists
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if need > free:
            raise ValueError(f"silhouette: the node sums ({s_bytes} bytes), the samples ({out_bytes} bytes) and the "
                             f"plan ({lists} bytes) need {need} bytes of device memory, {free} are free; sweep fewer "
                             f"n_clusters per call")
        to_dev = lambda a: torch.from_numpy(a).to(dev)
        node_ptr, members, sizes = to_dev(plan.node_ptr), to_dev(plan.members), to_dev(plan.sizes)
        cut_ptr, active, own = to_dev(plan.cut_ptr), to_dev(plan.active), to_dev(plan.own)
        square = need + 8 * n * n <= free
        dist = cond
        if square:
            dist = torch.empty((n, n), dtype=torch.float64, device=dev)
            _lib.call("expecto_square_distances", _lib.dptr(cond), n, _lib.dptr(dist))
        S = torch.empty((n_nodes, n), dtype=torch.float64, device=dev)
        samples = torch.empty((n_cuts, n), dtype=torch.float64, device=dev)
        _lib.call("expecto_silhouette_node_sums", _lib.dptr(dist), int(square), n, plan.node_ptr.ctypes.data,
                  _lib.dptr(node_ptr), _lib.dptr(members), n_nodes, _lib.dptr(S))
        _lib.call("expecto_silhouette_cuts", _lib.dptr(S), n, n_nodes, _lib.dptr(sizes), plan.cut_ptr.ctypes.data,
                  _lib.dptr(cut_ptr), _lib.dptr(active), _lib.dptr(own), n_cuts, _lib.dptr(samples))
        return samples.cpu().numpy()


def silhouette_sweep(children, condensed, n_leaves: int, ks):
    """``(scores float64 [len(ks)], samples float64 [len(ks), n])``: for every k of ``ks`` (distinct
    values of 2..n-1, any order) the silhouette samples of ``cut_tree(children, n_leaves, k)`` under
    the distances ``condensed`` (``pdist`` order; a device tensor, or a numpy array that is
    uploaded) and their mean -- sklearn's ``silhouette_samples`` / ``silhouette_score`` with
    ``metric='precomputed'``, bit for bit.  ValueError on a k out of range, a duplicate k, or a NaN /
    infinity among the distances."""
    n = int(n_leaves)
    plan = plan_sweep(children, n, ks)
    samples = _run_plan(_device_condensed(condensed, n), n, plan)
    return np.array([np.mean(row) for row in samples], np.float64), samples


def silhouette_samples(condensed, labels) -> np.ndarray:
    """sklearn's ``silhouette_samples(squareform(condensed), labels, metric='precomputed')`` (float64
    [n], its bits) for any integer ``labels`` with 2 to n - 1 distinct values."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.dtype.kind not in "iu":
        raise ValueError(f"silhouette_samples: labels must be a 1-D integer array, got {labels.dtype} {labels.shape}")
    n = labels.shape[0]
    values, inverse = np.unique(labels, return_inverse=True)
    if not 1 < len(values) < n:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % len(values))
    by_label = np.argsort(inverse, kind="stable")       # each cluster's points, ascending
    sizes = np.bincount(inverse)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    plan = SweepPlan(np.arange(len(values)), ptr, by_label.astype(np.int32), sizes.astype(np.int32),
                     np.array([0, len(values)], np.int64), np.arange(len(values), dtype=np.int32),
                     inverse.astype(np.int32).reshape(1, n))
    return _run_plan(_device_condensed(condensed, n), n, plan)[0]


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


def device_points(X_train: np.ndarray, n_marks: int, grouped: bool):
    """The points to cluster as a device tensor: the marks (grouped) or the 10 x marks features."""
    from . import _lib
    torch = _lib.require_gpu("interpret_features", " to cluster")
    x = torch.from_numpy(X_train).cuda()
    return features_grouped(x, n_marks) if grouped else x.T


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
    ks = None
    if args.silhouette is not None:
        k_min, k_max = args.silhouette[0], min(args.silhouette[1], n_points - 1)
        if k_min < 2 or k_min > k_max:
            raise ValueError(f"--silhouette {args.silhouette[0]} {args.silhouette[1]}: K_MIN must be at least 2 and "
                             f"at most K_MAX, which is clipped to n_points - 1 = {n_points - 1}")
        ks = list(range(k_min, k_max + 1))
    elif n_clusters == 'auto':
        raise ValueError("--n_clusters auto needs --silhouette K_MIN K_MAX")

    points = lambda: device_points(X_train, n_marks, args.grouped)
    condensed = None
    if args.clustering_joblib is None:
        print("Clustering and saving model to joblib..." if args.clustering_with_distances
              else "Clustering complete tree and caching...")
        if ks is None:
            children, distances = ward_tree(points())
        else:
            children, distances, condensed = ward_tree(points(), return_condensed=True)
        np.savez(f'{args.out_dir}/clustering.npz', children=children, distances=distances, n_leaves=n_points)
    else:
        print(f"Loading clustering model from {args.clustering_joblib}...")
        children, distances, n_leaves = load_tree(args.clustering_joblib)
        if n_leaves != n_points:
            raise ValueError(f"{args.clustering_joblib} holds a tree of {n_leaves} leaves, this run clusters "
                             f"{n_points} points")

    if ks is not None:
        if condensed is None:
            condensed = pairwise_condensed(points())
        scores, _ = silhouette_sweep(children, condensed, n_points, ks)
        del condensed
        with open(f'{args.out_dir}/silhouette_scores.tsv', 'w') as f:
            f.write('n_clusters\tsilhouette_score\n')
            f.writelines(f'{k}\t{float(score)!r}\n' for k, score in zip(ks, scores))
        best = int(np.argmax(scores))       # the first maximum: np.argmax(silhouette_scores) + 2 of the reference
        print(f"Best silhouette score: {float(scores[best])!r} at n_clusters={ks[best]}")
        if n_clusters == 'auto':
            n_clusters = ks[best]

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
