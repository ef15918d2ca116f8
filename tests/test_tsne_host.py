"""The host side of the t-SNE (no GPU): the numpy restatement of the contract (tests/tsne_ref.py)
against scikit-learn's recorded results (tests/golden/tsne, written by make_golden_tsne.py) and, where it
is installed, against scikit-learn itself; the pre-conditions that make the device tests'
bit-for-bit comparisons robust; the PCA start; and the refusals of ``cluster_and_viz.tsne``."""
import functools
import os

import numpy as np
import pytest

import tsne_ref
from conftest import GOLDEN
from expecto_amd import cluster_and_viz
from tsne_ref import KL_BOUND, Y_BOUND       # 100 x the measured values of test_restatement_against_sklearn

GOLD = os.path.join(GOLDEN, "tsne")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLD, "sklearn.npz")) as z:
        return {key: z[key] for key in z.files}


@functools.lru_cache(maxsize=None)
def restated(name):
    """(P, beta, steps, margin, Y, kl, iterations, checks) of a fixture case; shared, never changed."""
    X, Y0, kw = tsne_ref.case_inputs(name)
    kw = dict(kw)
    P, beta, steps, margin = tsne_ref.affinities(X, kw.pop("perplexity"))
    Y, kl, done, checks = tsne_ref.staged(P, Y0, **kw)
    for a in (P, beta, steps, Y):
        a.setflags(write=False)
    return P, beta, steps, margin, Y, kl, done, checks


def test_every_case_is_recorded():
    z = golden()
    assert sorted(z) == sorted(c + s for c in tsne_ref.CASES for s in ("_X", "_Y0", "_params", "_Y", "_kl", "_n_iter"))
    for name in tsne_ref.CASES:
        X, Y0, kw = tsne_ref.case_inputs(name)
        assert np.array_equal(X, z[name + "_X"]) and np.array_equal(Y0, z[name + "_Y0"])
        assert z[name + "_params"].tolist() == [kw["perplexity"], kw["early_exaggeration"], kw["learning_rate"],
                                                 kw["max_iter"]]
        D = tsne_ref.sqdist(X, X)
        assert np.array_equal(X, np.round(X)) and np.array_equal(D, D.astype(np.float32).astype(np.float64))


def compare(name, Y_want, kl_want, n_iter_want):
    _, _, _, _, Y, kl, done, _ = restated(name)
    dy = np.abs(Y - Y_want).max() / np.std(Y_want)
    dk = abs(kl - kl_want) / abs(kl_want)
    print(name, "max|dY|/std(Y)", dy, "kl rel", dk)
    assert done == n_iter_want + 1
    assert dy <= Y_BOUND and dk <= KL_BOUND, (name, dy, dk)


@pytest.mark.parametrize("name", tsne_ref.CASES)
def test_restatement_against_sklearn(name):
    """The restatement after the fixture's 300 iterations against sklearn 1.7.2's method='exact'.
    Measured (8 CPU threads, numpy 2.2.6): lattice60 max|dY|/std(Y) = 6.3e-16, kl equal;
    lattice130 max|dY|/std(Y) = 1.35e-8, kl relative 1.24e-10.  Both sides are float64 and differ in
    summation order (and in (12 P) / 12 for P in the second stage), amplified over 300 iterations; the
    bounds are 100 x the larger values."""
    assert Y_BOUND < 1e-3 and KL_BOUND < 1e-3
    z = golden()
    compare(name, z[name + "_Y"], float(z[name + "_kl"]), int(z[name + "_n_iter"]))


@pytest.mark.parametrize("name", tsne_ref.CASES)
def test_restatement_against_sklearn_live(name):
    pytest.importorskip("sklearn")
    from sklearn.manifold import TSNE
    X, Y0, kw = tsne_ref.case_inputs(name)
    ts = TSNE(n_components=2, method="exact", init=Y0.copy(), **kw)
    Y = ts.fit_transform(X.copy())
    compare(name, Y, float(ts.kl_divergence_), int(ts.n_iter_))


# ---- pre-conditions of the device tests ----------------------------------------------------------

def test_fixture_cases_are_robust_to_rounding():
    """No bisection branch and no stop decision of the fixture cases can flip under other ulps of exp
    and log: every |H - log(perplexity)| is at least 1e-9 from 0 and from the tolerance, and consecutive
    check-point errors differ by more than 1e-9 relative."""
    for name in tsne_ref.CASES:
        _, _, _, margin, _, _, _, checks = restated(name)
        assert margin >= 1e-9, (name, margin)
        errs = [c[1] for c in checks]
        assert len(errs) == 6
        assert min(abs(a - b) / abs(a) for a, b in zip(errs, errs[1:])) > 1e-9, name


def test_device_cases_are_robust_to_rounding():
    """The same margin on every input of tests/test_gpu_tsne.py's affinity cases."""
    import tsne_cases
    for key in tsne_cases.affinity_cases():
        _, _, steps, margin = tsne_cases.reference(key)
        assert margin >= 1e-9, (key, margin)
        assert steps.min() >= 1 and steps.max() <= 100
    # the duplicates' rows run all 100 steps; the spread-out input meets S == 0
    _, beta, steps, _ = tsne_cases.reference(("dup", 65, 20))
    assert (steps == 100).any() and (steps < 100).any()
    X, _ = tsne_cases.affinity_cases()[("far", 64, 1)]
    assert (np.exp(-tsne_ref.sqdist(X, X) + np.diag(np.full(64, -np.inf))).sum(axis=1) == 0.0).any()
    assert tsne_cases.full_scale_reference()[3] >= 1e-9


def test_wave_sum_order():
    """The restatement's sum is the header's: lane chains from +0.0, then the folds 32, 16, ..., 1."""
    rng = np.random.RandomState(0)
    for m in (1, 2, 63, 64, 65, 130, 200):
        a = rng.standard_normal(m) * 10.0 ** rng.randint(-8, 8, size=m)
        lanes = [0.0] * 64
        for j in range(m):
            lanes[j % 64] = lanes[j % 64] + a[j]
        for w in (32, 16, 8, 4, 2, 1):
            for l in range(w):
                lanes[l] = lanes[l] + lanes[l + w]
        assert tsne_ref.wave_sum(a) == lanes[0]
    assert tsne_ref.wave_sum(np.zeros((3, 0))).tolist() == [0.0, 0.0, 0.0]


def test_restatement_follows_sklearn_internals():
    """One step at a time against sklearn's own functions, where it is installed: the joint
    probabilities, and ten iterations of _gradient_descent under exaggeration."""
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    X, Y0, kw = tsne_ref.case_inputs("lattice60")
    n = X.shape[0]
    P = restated("lattice60")[0]
    Ps = squareform(_t_sne._joint_probabilities(tsne_ref.sqdist(X, X), kw["perplexity"], 0))
    assert np.abs(P - Ps).max() <= 64 * 2.0 ** -52 * Ps.max()
    p, err, it = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), it=0, max_iter=10, n_iter_check=5,
                                          momentum=0.5, learning_rate=3.0, n_iter_without_progress=10,
                                          args=[squareform(Ps) * 12.0, 1, n, 2], kwargs=dict(skip_num_points=0))
    Y, _, _, stats, _ = tsne_ref.descend(Ps, 12.0, Y0.copy(), np.zeros((n, 2)), np.ones((n, 2)), 0.5, 3.0, 10)
    assert it == 9 and np.abs(Y - p.reshape(n, 2)).max() <= 1e-10 * np.abs(Y).max()
    assert abs(stats[0] - err) <= 1e-12 * abs(err)


# ---- the start and the refusals ------------------------------------------------------------------

def test_pca_init_equals_sklearn_pca():
    X = tsne_ref.lattice(130, 20, 2)
    Y = cluster_and_viz.tsne_init(X, "pca")
    assert Y.shape == (130, 2) and Y.dtype == np.float64
    assert abs(np.std(Y[:, 0]) - 1e-4) <= 1e-18
    assert np.array_equal(Y, tsne_ref.pca_init(X))
    pytest.importorskip("sklearn")
    from sklearn.decomposition import PCA
    want = PCA(2, svd_solver="full").fit_transform(X)
    want = want / np.std(want[:, 0]) * 1e-4
    assert np.abs(Y - want).max() <= 1e-9 * np.abs(want).max()


def test_other_inits():
    X = tsne_ref.lattice(60, 5, 1)
    assert np.array_equal(cluster_and_viz.tsne_init(X, "random", seed=7),
                          1e-4 * np.random.RandomState(7).standard_normal((60, 2)))
    Y0 = tsne_ref.start(60, 3)
    got = cluster_and_viz.tsne_init(X, Y0)
    assert np.array_equal(got, Y0) and got is not Y0
    for bad in ("spectral", np.zeros((59, 2)), np.full((60, 2), np.nan)):
        with pytest.raises(ValueError, match="init"):
            cluster_and_viz.tsne_init(X, bad)
    with pytest.raises(ValueError, match="at least 2 dimensions"):
        cluster_and_viz.tsne_init(X[:, :1], "pca")
    assert cluster_and_viz.tsne_learning_rate(2002) == 50.0 and cluster_and_viz.tsne_learning_rate(4096, 4.0) == 256.0


def test_tsne_refuses_before_the_device():
    X = np.arange(15.0).reshape(5, 3)
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[1, 2] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            cluster_and_viz.tsne(Y, perplexity=2)
    with pytest.raises(ValueError, match="2-D"):
        cluster_and_viz.tsne(np.ones(5), perplexity=2)
    for shape in ((1, 3), (4097, 2), (5, 129)):
        with pytest.raises(ValueError, match="supported"):
            cluster_and_viz.tsne(np.ones(shape), perplexity=0.5)
    for perplexity in (5, 30.0, 0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="perplexity"):
            cluster_and_viz.tsne(X, perplexity=perplexity)
    with pytest.raises(ValueError, match="max_iter"):
        cluster_and_viz.tsne(X, perplexity=2, max_iter=0)
    with pytest.raises(ValueError, match="learning_rate"):
        cluster_and_viz.tsne(X, perplexity=2, learning_rate=0.0)
    with pytest.raises(ValueError, match="early_exaggeration"):
        cluster_and_viz.tsne(X, perplexity=2, early_exaggeration=0.5)
    with pytest.raises(ValueError, match="init"):
        cluster_and_viz.tsne(X, perplexity=2, init=np.zeros((4, 2)))


def test_cli_options():
    args = cluster_and_viz.build_parser().parse_args(["d", "--belugaFeatures", "f.tsv"])
    assert (args.tsne, args.tsne_perplexity, args.tsne_iter, args.tsne_init) == (False, 30.0, 1000, "pca")
    args = cluster_and_viz.build_parser().parse_args(["d", "--belugaFeatures", "f.tsv", "--tsne", "--tsne_perplexity", "5",
                                                      "--tsne_iter", "300", "--tsne_init", "random"])
    assert (args.tsne, args.tsne_perplexity, args.tsne_iter, args.tsne_init) == (True, 5.0, 300, "random")
