"""Exact t-SNE on the device: the kernels of csrc/tsne.hip through their C entry points,
``cluster_and_viz.tsne`` and the CLI's ``--tsne``.

One wave owns one row and lane l takes the columns l, l + 64, ...; the row kernels hold four rows per
workgroup.  The sizes below sit on both sides of a wave and of a workgroup's rows.  Outputs lie in
pattern-filled buffers (tests/guarded.py) and X inside NaN margins with NaN row padding (``ld > d``), so
a store outside an output or a load outside the matrix fails the test.  The bisection's decisions, and
with them beta and the step counts, and the whole descent are compared with the restatement
(tests/tsne_ref.py) by bits; P and the error, which pass through the device's exp and log, within the
ulp bounds stated at the comparisons.  tests/test_tsne_host.py checks that no input used here lets a
bisection branch depend on those ulps."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import kmeans_ref
import tsne_cases
import tsne_ref
from conftest import GOLDEN
from guarded import Guarded, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


class Rows64:
    """float64 [n, d] on the device with row stride ld; NaN padding, NaN margins before and after."""

    def __init__(self, X, ld, margin=64):
        X = np.asarray(X, np.float64)
        n, d = X.shape
        host = np.full(margin + n * ld + margin, np.nan)
        host[margin:margin + n * ld].reshape(n, ld)[:, :d] = X
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin
        self.n, self.d, self.ld = n, d, ld


def workspace(lib, n):
    nbytes = int(lib.expecto_tsne_workspace(n))
    assert nbytes > 0
    return Guarded((nbytes // 8,), np.float64), nbytes


def affinities_device(lib, X, perplexity, ld=None):
    n, d = X.shape
    src = Rows64(X, ld or d + 3)
    P, beta, steps = Guarded((n, n), np.float64), Guarded((n,), np.float64), Guarded((n,), np.int32)
    ws, nbytes = workspace(lib, n)
    st = lib.expecto_tsne_affinities(src.ptr, n, d, src.ld, perplexity, P.ptr, beta.ptr, steps.ptr, ws.ptr, nbytes, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    ws.result()
    return P.result(), beta.result(), steps.result()


class Descent:
    """The state of a descent in guarded buffers, for chained ``expecto_tsne_descend`` calls."""

    def __init__(self, lib, P, Y0):
        self.lib, self.n = lib, Y0.shape[0]
        self.P = dev(np.array(P, np.float64))
        self.Y, self.update, self.gains = (Guarded((self.n, 2), np.float64) for _ in range(3))
        self.Y.put(Y0)
        self.update.put(np.zeros((self.n, 2)))
        self.gains.put(np.ones((self.n, 2)))
        self.stats = Guarded((3,), np.float64)
        self.ws, self.nbytes = workspace(lib, self.n)

    def run(self, exaggeration, momentum, rate, n_iter, want_error=1):
        st = self.lib.expecto_tsne_descend(self.P.data_ptr(), self.n, exaggeration, self.Y.ptr, self.update.ptr,
                                           self.gains.ptr, momentum, rate, n_iter, want_error, self.stats.ptr,
                                           self.ws.ptr, self.nbytes, ST())
        assert st == 0, self.lib.expecto_last_error().decode()
        torch.cuda.synchronize()
        self.ws.result()
        return self.state()

    def state(self):
        return self.Y.result(), self.update.result(), self.gains.result(), self.stats.result()


def assert_state(got, want, mass, what):
    """Y, update, gains, the gradient norm and Z by bits; the error within 32 ulp of the sum of its terms'
    magnitudes (3 ulp of log and the product's rounding per term, with margin)."""
    for g, w, name in zip(got[:3], want[:3], ("Y", "update", "gains")):
        assert np.isfinite(w).all(), (what, name)
        assert_bits(g, np.ascontiguousarray(w), f"{what} {name}")
    assert_bits(got[3][1:], want[3][1:], what + " grad_norm, Z")
    diff = abs(got[3][0] - want[3][0])
    print(what, "error", got[3][0], "diff", diff, "allowed", 32 * ULP * mass)
    assert diff <= 32 * ULP * mass, (what, got[3][0], want[3][0])


# ---- affinities --------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(tsne_cases.affinity_cases()), ids=lambda k: f"{k[0]}-n{k[1]}-d{k[2]}")
def test_affinities(lib, key):
    X, perplexity = tsne_cases.affinity_cases()[key]
    want_P, want_beta, want_steps, _ = tsne_cases.reference(key)
    P, beta, steps = affinities_device(lib, X, perplexity)
    assert_bits(steps, want_steps, "steps")
    assert_bits(beta, want_beta, "beta")
    rel = np.abs(P - want_P).max() / want_P.max()
    print(key, "max |dP| / P", (np.abs(P - want_P) / np.where(want_P > 0, want_P, 1.0)).max(), "of max", rel)
    assert (np.abs(P - want_P) <= 64 * ULP * want_P).all()
    assert_bits(P, np.ascontiguousarray(P.T), "P symmetric")
    assert_bits(np.diag(P).copy(), np.zeros(X.shape[0]), "P diagonal")
    assert (P[~np.eye(X.shape[0], dtype=bool)] >= tsne_ref.EPS).all()
    if key[0] == "dup":
        assert steps[3] == 100 and steps.min() < 100
    if key == ("lat", 65, 20):        # the bits do not depend on the row stride
        again = affinities_device(lib, X, perplexity, ld=20)
        for g, w, name in zip(again, (P, beta, steps), ("P", "beta", "steps")):
            assert_bits(g, w, "ld = d " + name)


# ---- descent -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def descent_inputs(n):
    """(P, Y0): the restated affinities of the n-point lattice, and a start with point 1 on point 0."""
    P = tsne_cases.reference(("lat", n, 20))[0]
    Y0 = 100.0 * tsne_ref.start(n, n)
    Y0[1] = Y0[0]
    Y0.setflags(write=False)
    return P, Y0


@pytest.mark.parametrize("n", tsne_cases.NS)
def test_descent_bits(lib, n):
    P, Y0 = descent_inputs(n)
    run = Descent(lib, P, Y0)
    want = (np.array(Y0), np.zeros((n, 2)), np.ones((n, 2)))
    for call, (exaggeration, momentum) in enumerate([(12.0, 0.5)] * 3 + [(1.0, 0.8)] * 3):
        want = tsne_ref.descend(P, exaggeration, *want[:3], momentum, 20.0, 2)
        got = run.run(exaggeration, momentum, 20.0, 2)
        assert_state(got, want, want[4], f"n={n} call {call}")
        if call == 0 and n > 3:      # both gain branches were taken in the second iteration
            assert (want[2] == 1.0).any() and (want[2] == 0.8 * 0.8).any()


def test_descent_without_error(lib):
    """want_error = 0 leaves stats[0] alone and changes nothing else; an odd count ends in the caller's Y."""
    P, Y0 = descent_inputs(65)
    a, b = Descent(lib, P, Y0), Descent(lib, P, Y0)
    got = a.run(12.0, 0.5, 20.0, 3, want_error=0)
    ref = b.run(12.0, 0.5, 20.0, 3, want_error=1)
    for g, w in zip(got[:3], ref[:3]):
        assert_bits(g, w, "state")
    assert_bits(got[3][1:], ref[3][1:], "stats")
    assert (got[3][:1].view(np.uint8) == 0xA5).all()
    want = tsne_ref.descend(P, 12.0, np.array(Y0), np.zeros((65, 2)), np.ones((65, 2)), 0.5, 20.0, 3)
    assert_state(ref, want, want[4], "3 iterations")


def test_determinism(lib):
    """Two calls give equal bits; one call of 50 iterations equals 50 chained calls of one."""
    P, Y0 = descent_inputs(130)
    one, again, single = Descent(lib, P, Y0), Descent(lib, P, Y0), Descent(lib, P, Y0)
    a = one.run(12.0, 0.5, 20.0, 50)
    b = again.run(12.0, 0.5, 20.0, 50)
    for _ in range(50):
        c = single.run(12.0, 0.5, 20.0, 1)
    for x, y, z, name in zip(a, b, c, ("Y", "update", "gains", "stats")):
        assert np.isfinite(x).all()
        assert_bits(y, x, "second call " + name)
        assert_bits(z, x, "50 x 1 " + name)
    X, perplexity = tsne_cases.affinity_cases()[("lat", 130, 20)]
    for x, y in zip(affinities_device(lib, X, perplexity), affinities_device(lib, X, perplexity)):
        assert_bits(x, y, "affinities twice")


def test_full_scale(lib):
    """n = 2002, d = 20: the affinities' beta on a sample of rows, and six iterations of ``tsne`` across the
    stage switch (exploration_iter = 3, checks every 2) against the restated driver on the device's P."""
    from expecto_amd import cluster_and_viz
    X = tsne_cases.full_scale()
    rows = tsne_cases.FULL_ROWS
    _, want_beta, want_steps, _ = tsne_cases.full_scale_reference()
    P, beta, steps = cluster_and_viz.tsne_affinities(X, tsne_cases.FULL_PERPLEXITY)
    assert_bits(beta[rows], want_beta, "beta")
    assert_bits(steps[rows], want_steps, "steps")
    assert_bits(P, np.ascontiguousarray(P.T), "P symmetric")
    assert not np.diag(P).any() and abs(P.sum() - 1.0) < 1e-8
    Y0 = tsne_ref.pca_init(X)
    kw = dict(max_iter=6, exploration_iter=3, n_iter_check=2)
    got = cluster_and_viz.tsne(X, perplexity=tsne_cases.FULL_PERPLEXITY, init=Y0, **kw)
    want_Y, want_kl, done, _ = tsne_ref.staged(P, Y0, learning_rate=50.0, **kw)
    assert got.n_iter == done == 6
    assert_bits(got.embedding, want_Y, "embedding")
    assert_bits(got.beta, beta, "beta of tsne()")
    assert abs(got.kl_divergence - want_kl) <= 32 * ULP * 40.0      # sum |P log(P / Q)| <= sum P |log(eps)| < 40
    assert_bits(cluster_and_viz.tsne(X, perplexity=tsne_cases.FULL_PERPLEXITY, **kw).embedding, got.embedding, "pca init")


@pytest.mark.parametrize("name", tsne_ref.CASES)
def test_tsne_against_sklearn(name):
    """``tsne()`` after the fixture's 300 iterations against sklearn's recorded embedding, within the bound
    that the restatement meets (tests/test_tsne_host.py)."""
    from expecto_amd import cluster_and_viz
    with np.load(os.path.join(GOLDEN, "tsne", "sklearn.npz")) as z:
        X, Y0, want_Y, want_kl, n_iter = (z[name + s] for s in ("_X", "_Y0", "_Y", "_kl", "_n_iter"))
        perplexity, exaggeration, rate, max_iter = z[name + "_params"].tolist()
    timings = {}
    got = cluster_and_viz.tsne(X, perplexity=perplexity, early_exaggeration=exaggeration, learning_rate=rate,
                               max_iter=int(max_iter), init=Y0, timings=timings)
    dy = np.abs(got.embedding - want_Y).max() / np.std(want_Y)
    dk = abs(got.kl_divergence - float(want_kl)) / float(want_kl)
    print(name, "max|dY|/std(Y)", dy, "kl rel", dk, timings)
    assert got.n_iter == int(n_iter) + 1 == int(max_iter)
    assert dy <= tsne_ref.Y_BOUND and dk <= tsne_ref.KL_BOUND
    assert timings["affinities_ms"] > 0.0 and timings["descent_ms"] > 0.0
    assert got.embedding.shape == (X.shape[0], 2) and got.beta.shape == (X.shape[0],)


def test_stopping_rules():
    """The driver's two tests at the check points, against the restated driver on the device's P."""
    from expecto_amd import cluster_and_viz
    X, Y0, kw = tsne_ref.case_inputs("lattice60")
    P, _, _ = cluster_and_viz.tsne_affinities(X, kw["perplexity"])
    for extra in (dict(n_iter_check=10, min_grad_norm=0.05),
                  dict(n_iter_check=2, n_iter_without_progress=3, learning_rate=200.0, exploration_iter=0)):
        args = dict(kw, **extra)
        got = cluster_and_viz.tsne(X, init=Y0, **args)
        args.pop("perplexity")
        want_Y, _, done, checks = tsne_ref.staged(P, Y0, **args)
        errs = sorted(c[1] for c in checks)        # no decision hangs on the ulps of the error's log
        assert min(abs(a - b) / abs(a) for a, b in zip(errs, errs[1:])) > 1e-9
        assert min(abs(c[2] - args.get("min_grad_norm", 1e-7)) for c in checks) > 1e-9
        assert got.n_iter == done < 300, extra
        assert_bits(got.embedding, want_Y, str(extra))


# ---- refusals ----------------------------------------------------------------------------------

def test_refusals_and_nothing_to_do(lib):
    n, d = 65, 3
    X = tsne_ref.lattice(n, d, 1)
    src = Rows64(X, 4)
    P, beta, steps = Guarded((n, n), np.float64), Guarded((n,), np.float64), Guarded((n,), np.int32)
    Y, update, gains, stats = (Guarded(s, np.float64) for s in ((n, 2), (n, 2), (n, 2), (3,)))
    ws, nbytes = workspace(lib, n)
    Pd = dev(np.full((n, n), 1.0 / (n * n)))

    def aff(**k):
        a = dict(X=src.ptr, n=n, d=d, ld=4, perplexity=10.0, P=P.ptr, beta=beta.ptr, steps=steps.ptr, ws=ws.ptr,
                 nbytes=nbytes)
        a.update(k)
        return lib.expecto_tsne_affinities(*a.values(), ST())

    def des(**k):
        a = dict(P=Pd.data_ptr(), n=n, ex=12.0, Y=Y.ptr, update=update.ptr, gains=gains.ptr, mom=0.5, rate=50.0,
                 n_iter=2, want_error=1, stats=stats.ptr, ws=ws.ptr, nbytes=nbytes)
        a.update(k)
        return lib.expecto_tsne_descend(*a.values(), ST())

    for call, kw, text in (
            (aff, dict(n=1), "n must lie"), (aff, dict(n=4097), "n must lie"), (aff, dict(d=0), "d must lie"),
            (aff, dict(d=129, ld=129), "d must lie"), (aff, dict(ld=2), "ld < d"), (aff, dict(perplexity=0.0), "perplexity"),
            (aff, dict(perplexity=65.0), "perplexity"), (aff, dict(perplexity=float("nan")), "perplexity"),
            (aff, dict(X=None), "null argument"), (aff, dict(P=None), "null argument"), (aff, dict(beta=None), "null argument"),
            (aff, dict(steps=None), "null argument"), (aff, dict(ws=None), "null argument"),
            (aff, dict(nbytes=nbytes - 8), "workspace too small"), (aff, dict(ws=ws.ptr + 4), "8-byte aligned"),
            (des, dict(n=1), "n must lie"), (des, dict(n=4097), "n must lie"), (des, dict(n_iter=-1), "n_iter"),
            (des, dict(ex=float("inf")), "finite"), (des, dict(rate=float("nan")), "finite"),
            (des, dict(P=None), "null argument"), (des, dict(Y=None), "null argument"), (des, dict(update=None), "null argument"),
            (des, dict(gains=None), "null argument"), (des, dict(stats=None), "null argument"),
            (des, dict(ws=None), "null argument"), (des, dict(nbytes=nbytes - 8), "workspace too small"),
            (des, dict(n_iter=0, Y=None), "null argument")):
        assert call(**kw) == -1, (kw, text)
        assert text in lib.expecto_last_error().decode(), (kw, text, lib.expecto_last_error())
    assert lib.expecto_tsne_workspace(1) == 0 and lib.expecto_tsne_workspace(4097) == 0
    assert lib.expecto_tsne_workspace(4096) >= 8 * 6 * 4096
    assert des(n_iter=0) == 0          # nothing to do: nothing written
    torch.cuda.synchronize()
    for g in (P, beta, steps, Y, update, gains, stats, ws):
        assert g.untouched()
    # the good arguments do run
    Y.put(tsne_ref.start(n, 1))
    update.put(np.zeros((n, 2)))
    gains.put(np.ones((n, 2)))
    assert aff() == 0 and des() == 0
    torch.cuda.synchronize()
    assert not P.untouched() and not stats.untouched()


def test_api_refusals():
    from expecto_amd.cluster_and_viz import tsne
    with pytest.raises(ValueError, match="perplexity"):
        tsne(np.arange(10.0).reshape(5, 2), perplexity=5)
    with pytest.raises(ValueError, match="NaN or infinity"):
        tsne(np.full((5, 2), np.inf), perplexity=2)


# ---- CLI -------------------------------------------------------------------------------------

def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_tsne(tmp_path, capsys):
    """``--tsne`` adds its files beside the k-means files, which stay byte-equal to the reference run's."""
    import json

    from expecto_amd import cluster_and_viz
    gold = os.path.join(GOLDEN, "kmeans", "cli")
    src = tmp_path / "in"
    src.mkdir()
    Xr = kmeans_ref.cli_reduced(kmeans_ref.CLI_MARKS)
    np.save(src / "tf_idf_reduced_100.npy", Xr)
    out = tmp_path / "out"
    capsys.readouterr()
    cluster_and_viz.main([str(src), "--belugaFeatures", FEATURES_TSV, *kmeans_ref.CLI_FLAGS, "-o", str(out), "--seed", "0",
                          "--tsne", "--tsne_iter", "100", "--tsne_perplexity", "20"])
    assert capsys.readouterr().out.encode() == read(os.path.join(gold, "stdout.txt"))
    for name in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
        assert read(out / name) == read(os.path.join(gold, name)), name
    clusters = b"".join(f"== cluster_{i}.tsv\n".encode() + read(out / "clusters" / f"cluster_{i}.tsv") for i in range(30))
    assert clusters == read(os.path.join(gold, "clusters.txt"))
    table = pd.read_csv(out / "tsne_embedding.tsv", sep="\t", index_col=0)
    want = pd.read_csv(os.path.join(gold, "all_feature_clusters.tsv"), sep="\t", index_col=0)
    assert list(table.columns) == ["tsne_0", "tsne_1", "cluster"]
    assert table.index.tolist() == want.index.tolist() and table["cluster"].tolist() == want["cluster"].tolist()
    res = cluster_and_viz.tsne(Xr[:, :20], perplexity=20.0, max_iter=100, init="pca", seed=0)
    lines = read(out / "tsne_embedding.tsv").decode().splitlines()[1:]
    assert [ln.split("\t")[1:3] for ln in lines] == [[repr(float(a)), repr(float(b))] for a, b in res.embedding]
    meta = json.loads(read(out / "tsne.json"))
    assert meta == {"kl_divergence": res.kl_divergence, "n_iter": 100, "perplexity": 20.0, "learning_rate": 50.0,
                    "init": "pca", "seed": 0}
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert not (out / "tsne.png").exists()
    else:
        assert read(out / "tsne.png")[:8] == b"\x89PNG\r\n\x1a\n"
    # without the flag: none of the three files
    plain = tmp_path / "plain"
    cluster_and_viz.main([str(src), "--belugaFeatures", FEATURES_TSV, *kmeans_ref.CLI_FLAGS, "-o", str(plain)])
    assert not [f for f in os.listdir(plain) if f.startswith("tsne")]
