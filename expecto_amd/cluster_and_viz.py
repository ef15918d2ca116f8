"""Drop-in for the reference ``cluster_and_viz.py``: k-means of the marks' SVD coordinates
(``tf_idf_reduced_100.npy`` of ``expecto_amd.svd``) on the GPU, and the cluster files that
``predict_by_cluster --feature_clusters_df`` reads.

    python -m expecto_amd.cluster_and_viz <svd_transform_dir> --belugaFeatures features.tsv [ablation flags] \\
        [-o temp_cluster_and_viz] [--n_pcs 20] [--n_clusters 30] [--n_init 1] [--seed 0] [--elbow K_MIN K_MAX STEP] \\
        [--tsne] [--tsne_perplexity 30] [--tsne_iter 1000] [--tsne_init pca|random]

The reference runs ``KMeans(n_clusters=30)`` after ``np.random.seed(0)`` on the first 20 coordinates.
Here the seeding (sklearn's greedy k-means++) and the Lloyd iteration run on the device
(``expecto_kmeans_plusplus``, ``expecto_kmeans_lloyd``) in float64 with a fixed order of every sum
(include/expecto_hip.h); the random numbers are drawn on the host in sklearn's order
(:func:`kmeans_draws`), so ``--seed 0`` consumes the stream the reference consumes.  ``--elbow`` is the
sweep the reference has commented out (``for k in range(2, 200, 5)``): every ``(k, restart)`` is one
problem of a single seeding call and a single Lloyd call.

``--tsne`` adds the reference's picture, ``TSNE(n_components=2, random_state=0).fit_transform(X)`` coloured
by cluster: exact t-SNE on the device (:func:`tsne`; ``expecto_tsne_affinities``, ``expecto_tsne_descend``)
where sklearn defaults to the Barnes-Hut approximation, written as ``tsne_embedding.tsv``, ``tsne.json``
and, if matplotlib is installed, ``tsne.png`` (saved, never shown).  Off by default.

Differences from the reference, on purpose:
* float64 arithmetic on the file's float32 values (sklearn computes in float32 through BLAS there);
* the t-SNE picture is opt-in (``--tsne``), exact rather than Barnes-Hut, starts from a full SVD's
  principal scores kept in float64 (sklearn: a randomized PCA cast to float32), and goes to files;
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
    from . import _lib
    torch = _lib.require_gpu("cluster_and_viz")
    lib = _lib.load()
    dev = _lib.device_of(device)
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
    with torch.cuda.device(dev):
        Xd, ud, seed_d, lloyd_d = (_lib.upload(a, dev) for a in (X, u, seed_tab, lloyd_tab))
        told = torch.full((P,), float(tol), dtype=torch.float64, device=dev)
        total = int(c_off[-1])
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        init = torch.empty((total, d), dtype=torch.float64, device=dev)
        centres = torch.empty((total, d), dtype=torch.float64, device=dev)
        labels = torch.empty((P, n), dtype=torch.int32, device=dev)
        inertia = torch.empty(P, dtype=torch.float64, device=dev)
        n_iter = torch.empty(P, dtype=torch.int32, device=dev)
        ws = _lib.workspace(nbytes, dev)
        timer = _lib.EventTimer(timings)
        timer.mark()
        _lib.call("expecto_kmeans_plusplus", Xd.data_ptr(), n, d, d, P, seed_tab.ctypes.data, seed_d.data_ptr(),
                  ud.data_ptr(), idx.data_ptr(), init.data_ptr(), ws.data_ptr(), nbytes)
        timer.mark()
        _lib.call("expecto_kmeans_lloyd", Xd.data_ptr(), n, d, d, P, lloyd_tab.ctypes.data, lloyd_d.data_ptr(),
                  told.data_ptr(), init.data_ptr(), labels.data_ptr(), centres.data_ptr(), inertia.data_ptr(),
                  n_iter.data_ptr(), ws.data_ptr(), nbytes)
        timer.mark()
        idx, centres, labels = idx.cpu().numpy(), centres.cpu().numpy(), labels.cpu().numpy()
        inertia, n_iter = inertia.cpu().numpy(), n_iter.cpu().numpy()
        timer.set("seeding_ms", 0)
        timer.set("lloyd_ms", 1)
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


# ---- t-SNE -----------------------------------------------------------------------------------

class TSNEResult(NamedTuple):
    embedding: np.ndarray     # float64 [n, 2]
    kl_divergence: float      # of the last iteration run
    n_iter: int               # iterations run (sklearn's n_iter_ is the last one's index, one less)
    beta: np.ndarray          # float64 [n]: the precision 1 / (2 sigma_i^2) the perplexity search found per point


def _tsne_checked(X, perplexity):
    X = np.array(X, dtype=np.float64, order='C')
    if X.ndim != 2:
        raise ValueError(f"tsne: X must be 2-D, got shape {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError("tsne: X contains NaN or infinity")
    n, d = X.shape
    if not (2 <= n <= MAX_N and 1 <= d <= MAX_D):
        raise ValueError(f"tsne: X has shape {X.shape}; supported are 2..{MAX_N} points of 1..{MAX_D} dimensions")
    perplexity = float(perplexity)
    if not 0.0 < perplexity < n:
        raise ValueError(f"tsne: perplexity = {perplexity} outside (0, n) with n = {n}")
    return X, perplexity


def tsne_init(X, init='pca', seed=0):
    """The initial embedding, float64 [n, 2], on the host.  ``'pca'``: the first two principal scores from
    numpy's SVD of the centred X with sklearn's sign convention (``svd_flip`` decided on v), scaled to a
    standard deviation of 1e-4 along the first; ``'random'``: ``1e-4 * RandomState(seed).standard_normal``;
    an [n, 2] array is taken as given."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    if isinstance(init, str):
        if init == 'random':
            return 1e-4 * np.random.RandomState(seed).standard_normal((n, 2))
        if init != 'pca':
            raise ValueError(f"tsne: init = {init!r}; supported are 'pca', 'random' and an [n, 2] array")
        if X.shape[1] < 2:
            raise ValueError("tsne: init='pca' needs at least 2 dimensions")
        U, S, Vt = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)
        signs = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
        Y = (U * signs)[:, :2] * S[:2]
        return Y / np.std(Y[:, 0]) * 1e-4
    Y = np.array(init, dtype=np.float64)
    if Y.shape != (n, 2) or not np.isfinite(Y).all():
        raise ValueError(f"tsne: init must be a finite [{n}, 2] array, got shape {Y.shape}")
    return Y


def tsne_learning_rate(n, early_exaggeration=12.0):
    """sklearn's ``learning_rate='auto'``."""
    return float(max(n / early_exaggeration / 4, 50))


class _TsneDevice:
    """The device side of one embedding: X's affinities, then chained descent calls on resident buffers."""

    def __init__(self, X, perplexity, device=None, timed=False):
        from . import _lib
        torch = _lib.require_gpu("cluster_and_viz")
        self.torch, self._lib = torch, _lib
        self.dev = _lib.device_of(device)
        self.n = X.shape[0]
        self.ms = {"affinities_ms": 0.0, "descent_ms": 0.0} if timed else None    # summed over this embedding's calls
        n, d = X.shape
        self.nbytes = int(_lib.load().expecto_tsne_workspace(n))
        with torch.cuda.device(self.dev):
            f64 = dict(dtype=torch.float64, device=self.dev)
            Xd = torch.from_numpy(X).to(self.dev)
            self.P, self.beta = torch.empty((n, n), **f64), torch.empty(n, **f64)
            self.steps = torch.empty(n, dtype=torch.int32, device=self.dev)
            self.ws = _lib.workspace(self.nbytes, self.dev)
            self.Y, self.update, self.gains = (torch.empty((n, 2), **f64) for _ in range(3))
            self.stats = torch.zeros(3, **f64)
            self._timed("affinities_ms", "expecto_tsne_affinities", Xd.data_ptr(), n, d, d, perplexity,
                        self.P.data_ptr(), self.beta.data_ptr(), self.steps.data_ptr(), self.ws.data_ptr(), self.nbytes)

    def _timed(self, key, name, *args):
        timer = self._lib.EventTimer(self.ms)
        timer.mark()
        self._lib.call(name, *args)
        timer.mark(sync=True)
        timer.add(key)

    def start(self, Y0):
        with self.torch.cuda.device(self.dev):
            self.Y.copy_(self.torch.from_numpy(np.ascontiguousarray(Y0)))

    def reset(self):
        self.update.zero_()
        self.gains.fill_(1.0)

    def descend(self, exaggeration, momentum, learning_rate, n_iter):
        """n_iter iterations; returns the call's (error, grad_norm, Z)."""
        with self.torch.cuda.device(self.dev):
            self._timed("descent_ms", "expecto_tsne_descend", self.P.data_ptr(), self.n, float(exaggeration),
                        self.Y.data_ptr(), self.update.data_ptr(), self.gains.data_ptr(), float(momentum),
                        float(learning_rate), int(n_iter), 1, self.stats.data_ptr(), self.ws.data_ptr(), self.nbytes)
            return self.stats.cpu().numpy()


def tsne_affinities(X, perplexity=30.0, device=None):
    """``expecto_tsne_affinities`` of X on the device: (P float64 [n, n], beta float64 [n], steps int32 [n])
    as host arrays -- sklearn's joint probabilities in full-matrix form."""
    X, perplexity = _tsne_checked(X, perplexity)
    t = _TsneDevice(X, perplexity, device=device)
    return t.P.cpu().numpy(), t.beta.cpu().numpy(), t.steps.cpu().numpy()


def tsne(X, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000, init='pca', seed=0,
         exploration_iter=250, n_iter_check=50, n_iter_without_progress=300, min_grad_norm=1e-7, device=None,
         timings=None) -> TSNEResult:
    """``TSNE(n_components=2, method='exact', ...).fit_transform(X)`` on the device: the affinities in one
    call, then sklearn's two stages (momentum 0.5 under ``early_exaggeration`` for ``exploration_iter``
    iterations, then momentum 0.8) in chunks that end at its check points, every ``n_iter_check`` iterations,
    where the host applies sklearn's two stopping tests to the chunk's statistics.  ``timings``: a dict
    that receives the event-timed device ms of the affinity call and of all descent calls
    (``affinities_ms``, ``descent_ms``).  ``ValueError`` for unsupported input, before the device is touched."""
    X, perplexity = _tsne_checked(X, perplexity)
    n = X.shape[0]
    max_iter, exploration_iter, n_iter_check = int(max_iter), int(exploration_iter), int(n_iter_check)
    if max_iter < 1 or exploration_iter < 0 or n_iter_check < 1:
        raise ValueError("tsne: max_iter and n_iter_check must be at least 1, exploration_iter at least 0")
    early_exaggeration = float(early_exaggeration)
    if not (np.isfinite(early_exaggeration) and early_exaggeration >= 1.0):
        raise ValueError("tsne: early_exaggeration must be a finite number of at least 1")
    if isinstance(learning_rate, str):
        if learning_rate != 'auto':
            raise ValueError("tsne: learning_rate must be 'auto' or a positive number")
        learning_rate = tsne_learning_rate(n, early_exaggeration)
    learning_rate = float(learning_rate)
    if not (np.isfinite(learning_rate) and learning_rate > 0.0):
        raise ValueError("tsne: learning_rate must be 'auto' or a positive number")
    Y0 = tsne_init(X, init, seed)

    t = _TsneDevice(X, perplexity, device=device, timed=timings is not None)
    t.start(Y0)
    done, kl = 0, float('nan')
    for end, momentum, exaggeration, window in ((min(exploration_iter, max_iter), 0.5, early_exaggeration, exploration_iter),
                                                (max_iter, 0.8, 1.0, int(n_iter_without_progress))):
        t.reset()       # sklearn calls _gradient_descent afresh for each stage
        best, best_iter = np.finfo(np.float64).max, done
        while done < end:
            nxt = min(end, (done // n_iter_check + 1) * n_iter_check)
            kl, grad_norm, _ = (float(v) for v in t.descend(exaggeration, momentum, learning_rate, nxt - done))
            done = nxt
            if done % n_iter_check == 0:
                if kl < best:
                    best, best_iter = kl, done - 1
                elif done - 1 - best_iter > window:
                    break
                if grad_norm <= min_grad_norm:
                    break
    if timings is not None:
        timings.update(t.ms)
    return TSNEResult(t.Y.cpu().numpy(), kl, done, t.beta.cpu().numpy())


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
    parser.add_argument('--tsne', action='store_true', default=False,
                        help='also embed the marks in two dimensions (exact t-SNE): tsne_embedding.tsv, tsne.json, tsne.png')
    parser.add_argument('--tsne_perplexity', type=float, default=30.0)
    parser.add_argument('--tsne_iter', type=int, default=1000, help='iterations of the t-SNE descent at most')
    parser.add_argument('--tsne_init', choices=('pca', 'random'), default='pca')
    return parser


def write_tsne(args, X, input_features_df, labels, k):
    """The files of ``--tsne`` (cluster_and_viz.py:60-67; the picture is saved, not shown)."""
    import json

    rate = tsne_learning_rate(X.shape[0])
    res = tsne(X, perplexity=args.tsne_perplexity, learning_rate=rate, max_iter=args.tsne_iter, init=args.tsne_init,
               seed=args.seed)
    with open(f'{args.out_dir}/tsne_embedding.tsv', 'w') as f:
        f.write('\ttsne_0\ttsne_1\tcluster\n')
        f.writelines(f'{ix}\t{float(y[0])!r}\t{float(y[1])!r}\t{int(c)}\n'
                     for ix, y, c in zip(input_features_df.index, res.embedding, labels))
    with open(f'{args.out_dir}/tsne.json', 'w') as f:
        json.dump({'kl_divergence': res.kl_divergence, 'n_iter': res.n_iter, 'perplexity': args.tsne_perplexity,
                   'learning_rate': rate, 'init': args.tsne_init, 'seed': args.seed}, f, indent=1)
        f.write('\n')
    try:
        import matplotlib
    except ImportError:
        return res
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig = plt.figure()
    for i in range(k):
        X_plot = res.embedding[labels == i]
        plt.scatter(X_plot[:, 0], X_plot[:, 1], label=f'cluster {i}')
    fig.savefig(f'{args.out_dir}/tsne.png')
    plt.close(fig)
    return res


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
    if args.tsne:
        write_tsne(args, X, input_features_df, labels, k)

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
