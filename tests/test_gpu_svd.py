"""The tf-idf SVD on the device: the kernels of svd.hip through their C entry points, then
``expecto_amd.svd.fit`` / ``transform`` and the ``python -m expecto_amd.svd`` CLI.

The Gram, projection and transform kernels work on 64 x 64 tiles (TILE) and stage 32 columns (or
marks) at a time (STAGE); the shapes below sit on both sides of both.  Outputs lie in pattern-filled
buffers (tests/guarded.py); the track chunk lies in a NaN-filled buffer with ``ld`` > marks and every
mark that is not kept is NaN, so a wrong gather or a load from the padding poisons the result.
Every bound is the worst-case rounding error of a float64 sum in any order, computed from the
restatement (tests/svd_ref.py)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import svd_ref
from conftest import GOLDEN
from guarded import Guarded, Margined, ST, dev

pytestmark = pytest.mark.gpu

TILE, STAGE = 64, 32
U = 2.0 ** -53
# More stages than the column split ever makes parts (64), so every workgroup walks several stages:
# the prefetch of the next stage and the reuse of the staging registers run with a checked result.
N_LONG = 64 * STAGE * 2 + 33
FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
GOLD = os.path.join(GOLDEN, "svd")
LEADING = 16


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


class Chunk:
    """n columns of m kept marks among 2 m + 3 marks: the kept ones ascending with gaps (``m`` odd) or
    reversed (``m`` even).  Values in (0, 1) with exact zeros; column 1 is all zero (idf = log m) and
    column 2 lies within 1e-3 of 1 (c_n > m - 1: a negative idf) where n allows.  Everything that is
    not a kept mark's value is NaN."""

    def __init__(self, m, n, seed=0):
        rng = np.random.default_rng([m, n, seed])
        self.m, self.n, self.marks = m, n, 2 * m + 3
        self.ld = self.marks + 5
        keep = 1 + 2 * np.arange(m) + (np.arange(m) > m // 2)
        self.keep = np.ascontiguousarray(keep[::-1] if m % 2 == 0 else keep).astype(np.int32)
        x = rng.random((n, m)).astype(np.float32)
        x[rng.random((n, m)) < 0.1] = 0.0
        if n > 2:
            x[1] = 0.0
            x[2] = (1.0 - 1e-3 * rng.random(m)).astype(np.float32)
        self.X = np.full((n, self.marks), np.nan, np.float32)
        self.X[:, self.keep] = x
        self.D = Margined(self.X, self.ld, 64)
        self.keep_dev = dev(self.keep)
        self.w = svd_ref.idf(self.X, self.keep)
        self.w_dev = dev(self.w)

    def args(self, n=None):
        return (self.D.ptr, self.n if n is None else n, self.ld, self.keep_dev.data_ptr(), self.m)


def ok(lib, st):
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()


# ---- stats -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 31, 33, 257])
@pytest.mark.parametrize("m", [1, 17, 64, 65])
def test_stats(lib, m, n):
    c = Chunk(m, n)
    idf = Guarded((n,), np.float64)
    prefill = np.random.default_rng(m).normal(size=m)
    rs = Guarded((m,), np.float64).put(prefill)
    ok(lib, lib.expecto_tfidf_stats(*c.args(), idf.ptr, rs.ptr, ST()))
    got_idf, got_rs = idf.result(), rs.result()
    err = np.abs(got_idf - c.w)
    print(f"stats m={m} n={n}: idf err {err.max():.3g}")
    assert (err <= (m + 4) * 2 * U * np.maximum(1.0, np.abs(c.w))).all()
    if n > 2:
        assert c.w[1] == np.log(float(m)) and c.w[2] < 0 and got_idf[2] < 0
    x = svd_ref.kept(c.X, c.keep)
    want = x.sum(axis=0)
    err = np.abs(got_rs - prefill - want)
    print(f"stats m={m} n={n}: row sum err {err.max():.3g}")
    # the issue's bound on the sum, plus the one rounding of adding it to the prefilled value
    assert (err <= n * U * np.abs(x).sum(axis=0) + 2 * U * np.abs(prefill + want)).all()


# ---- Gram ------------------------------------------------------------------------------------

def run_gram(lib, c, H, n=None, first=0):
    n = c.n if n is None else n
    nbytes = lib.expecto_tfidf_gram_workspace(c.m, n)
    assert nbytes == lib.expecto_tfidf_gram_parts(c.m, n) * ((c.m + TILE - 1) // TILE) * \
        ((c.m + TILE - 1) // TILE + 1) // 2 * TILE * TILE * 8
    ws = Guarded((nbytes // 8,), np.float64)
    ok(lib, lib.expecto_tfidf_gram(c.D.ptr + 4 * first * c.ld, n, c.ld, c.keep_dev.data_ptr(), c.m,
                                   c.w_dev.data_ptr() + 8 * first, H.ptr, ws.ptr, nbytes, ST()))
    ws.result()     # nothing written around the workspace
    return H.result()


@pytest.mark.parametrize("n", [1, 31, 33, 257, N_LONG])
@pytest.mark.parametrize("m", [1, 17, 64, 65, 127, 130])
def test_gram(lib, m, n):
    """m: one tile, tile +- 1, three tile rows; n: a stage +- 1, many stages plus a tail.  n = 257
    splits into >= 3 parts whose last one is shorter (one stage per part); at N_LONG every part
    holds several stages, the last part fewer and a one-column tail.

    The bounds of the prefilled and of the two-chunk run are the issue's bound plus
    2 U |H0 + want|: the one more rounding of adding a chunk's sum into what H_acc held, which the
    worst-case bound of the sum itself does not cover (at n = 1 that sum is one exact product's
    rounding)."""
    c = Chunk(m, n)
    if n == 257:
        assert lib.expecto_tfidf_gram_parts(m, n) >= 3 and n % STAGE != 0
    if n == N_LONG:
        assert lib.expecto_tfidf_gram_parts(m, n) * STAGE * 2 <= n      # at least two stages in every full part
    want, scale = svd_ref.gram(c.X, c.keep, c.w), svd_ref.gram_abs(c.X, c.keep, c.w)
    bound = 2 * n * U * scale
    got = run_gram(lib, c, Guarded((m, m), np.float64).put(np.zeros((m, m))))
    print(f"gram m={m} n={n}: max err / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3g}")
    assert (np.abs(got - want) <= bound).all()
    assert np.array_equal(got, got.T) and (np.diag(got) >= 0).all()
    again = run_gram(lib, c, Guarded((m, m), np.float64).put(np.zeros((m, m))))
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))        # the same bits
    # accumulation into a prefilled H, and two chunks against one call
    H0 = np.random.default_rng(n).normal(size=(m, m))
    H0 = H0 + H0.T
    got = run_gram(lib, c, Guarded((m, m), np.float64).put(H0))
    assert (np.abs(got - H0 - want) <= bound + 2 * U * np.abs(H0 + want)).all() and np.array_equal(got, got.T)
    if n > 1:
        H = Guarded((m, m), np.float64).put(np.zeros((m, m)))
        a = n // 3 + 1
        run_gram(lib, c, H, n=a)
        got = run_gram(lib, c, H, n=n - a, first=a)
        assert (np.abs(got - want) <= bound + 2 * U * np.abs(want)).all() and np.array_equal(got, got.T)


# ---- project and transform -------------------------------------------------------------------

PT_SHAPES = [(1, 1, 1), (17, 31, 8), (64, 33, 17), (65, 257, 8), (127, 65, 1), (130, 257, 17), (17, 130, 65),
             (17, N_LONG, 8), (65, N_LONG, 17)]


@pytest.mark.parametrize("m,n,k", PT_SHAPES)
def test_project(lib, m, n, k):
    c = Chunk(m, n)
    P = np.random.default_rng([m, n, k]).normal(size=(k, m))
    ld_out = n + 3
    out = Guarded((k, ld_out), np.float32)
    ok(lib, lib.expecto_tfidf_project(*c.args(), c.w_dev.data_ptr(), dev(P).data_ptr(), k, out.ptr, ld_out, ST()))
    got = out.result()
    assert (got[:, n:].view(np.uint32) == 0xA5A5A5A5).all()      # the rows' padding is not written
    want = svd_ref.project(c.X, c.keep, c.w, P)
    bound64 = 2 * m * U * (np.abs(P) @ svd_ref.kept(c.X, c.keep).T) * np.abs(c.w)[None, :]
    want32 = want.astype(np.float32)
    err = np.abs(got[:, :n].astype(np.float64) - want32)
    print(f"project {m}x{n}x{k}: max err {err.max():.3g}")
    assert (err <= np.spacing(np.abs(want32)).astype(np.float64) + bound64).all()


@pytest.mark.parametrize("m,n,k", PT_SHAPES)
def test_transform(lib, m, n, k):
    c = Chunk(m, n)
    rng = np.random.default_rng([k, n, m])
    V = rng.normal(size=(k, n)).astype(np.float32)
    Vd = Margined(V, n + 2, 64)
    X0 = rng.normal(size=(m, k))
    nbytes = lib.expecto_tfidf_transform_workspace(m, k, n)
    assert nbytes == lib.expecto_tfidf_transform_parts(m, k, n) * ((m + TILE - 1) // TILE) * ((k + TILE - 1) // TILE) * \
        TILE * TILE * 8
    if n == 257:
        assert lib.expecto_tfidf_transform_parts(m, k, n) >= 3
    if n == N_LONG:     # every full part holds at least two stages: the stage loop iterates
        assert lib.expecto_tfidf_transform_parts(m, k, n) * STAGE * 2 <= n
    ws = Guarded((nbytes // 8,), np.float64)
    X = Guarded((m, k), np.float64).put(X0)
    ok(lib, lib.expecto_tfidf_transform(*c.args(), c.w_dev.data_ptr(), Vd.ptr, n + 2, k, X.ptr, ws.ptr, nbytes, ST()))
    ws.result()
    got = X.result()
    want = svd_ref.transform(c.X, c.keep, V, c.w, scale=False)
    bound = 2 * n * U * (np.abs(svd_ref.tvalues(c.X, c.keep, c.w)).T @ np.abs(V.astype(np.float64)).T)
    err = np.abs(got - X0 - want)
    print(f"transform {m}x{n}x{k}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    # the sum's worst-case bound, plus the one rounding of adding it to the prefilled X_acc
    assert (err <= bound + 2 * U * np.abs(X0 + want)).all()


# ---- refusals and no-ops ---------------------------------------------------------------------

def test_refusals_and_no_ops(lib):
    c = Chunk(17, 33)
    m, n, k = c.m, c.n, 4
    D, keep, w = c.D.ptr, c.keep_dev.data_ptr(), c.w_dev.data_ptr()
    idf, rs = Guarded((n,), np.float64), Guarded((m,), np.float64)
    H, X = Guarded((m, m), np.float64), Guarded((m, k), np.float64)
    out = Guarded((k, n), np.float32)
    P, V = dev(np.ones((k, m))), dev(np.ones((k, n), np.float32))
    gb, tb = lib.expecto_tfidf_gram_workspace(m, n), lib.expecto_tfidf_transform_workspace(m, k, n)
    ws = Guarded((max(gb, tb) // 8,), np.float64)
    s = ST()
    stats = lambda **o: lib.expecto_tfidf_stats(*[o.get(a, v) for a, v in (
        ("D", D), ("n", n), ("ld", c.ld), ("keep", keep), ("m", m), ("idf", idf.ptr), ("rs", rs.ptr))], s)
    gram = lambda **o: lib.expecto_tfidf_gram(*[o.get(a, v) for a, v in (
        ("D", D), ("n", n), ("ld", c.ld), ("keep", keep), ("m", m), ("w", w), ("H", H.ptr), ("ws", ws.ptr),
        ("bytes", gb))], s)
    project = lambda **o: lib.expecto_tfidf_project(*[o.get(a, v) for a, v in (
        ("D", D), ("n", n), ("ld", c.ld), ("keep", keep), ("m", m), ("w", w), ("P", P.data_ptr()), ("k", k),
        ("out", out.ptr), ("ld_out", n))], s)
    transform = lambda **o: lib.expecto_tfidf_transform(*[o.get(a, v) for a, v in (
        ("D", D), ("n", n), ("ld", c.ld), ("keep", keep), ("m", m), ("w", w), ("V", V.data_ptr()), ("ld_v", n), ("k", k),
        ("X", X.ptr), ("ws", ws.ptr), ("bytes", tb))], s)
    cases = [(stats, dict(D=None), "null argument"), (stats, dict(idf=None), "null argument"),
             (stats, dict(rs=None), "null argument"), (stats, dict(keep=None), "null argument"),
             (stats, dict(n=-1), "negative shape"), (stats, dict(m=-1), "negative shape"),
             (stats, dict(ld=m - 1), "ld < m"),
             (gram, dict(D=None), "null argument"), (gram, dict(w=None), "null argument"),
             (gram, dict(H=None), "null argument"), (gram, dict(ws=None), "null argument"),
             (gram, dict(n=-1), "negative shape"), (gram, dict(ld=m - 1), "ld < m"),
             (gram, dict(bytes=gb - 1), "workspace smaller"),
             (project, dict(P=None), "null argument"), (project, dict(out=None), "null argument"),
             (project, dict(k=-1), "negative shape"), (project, dict(ld=m - 1), "ld < m"),
             (project, dict(ld_out=n - 1), "ld_out < n"),
             (transform, dict(V=None), "null argument"), (transform, dict(X=None), "null argument"),
             (transform, dict(k=-1), "negative shape"), (transform, dict(ld_v=n - 1), "ld_v < n"),
             (transform, dict(ld=m - 1), "ld < m"), (transform, dict(bytes=tb - 1), "workspace smaller")]
    for fn, override, text in cases:
        assert fn(**override) == -1, (override, text)
        assert text in lib.expecto_last_error().decode(), (override, lib.expecto_last_error())
    for fn in (stats, gram, project, transform):       # nothing to do: even null pointers pass
        assert fn(n=0) == 0 and fn(m=0, ld=c.ld) == 0
        assert fn(n=0, D=None, keep=None) == 0
    assert project(k=0) == 0 and transform(k=0) == 0
    assert lib.expecto_tfidf_gram_parts(0, 5) == 0 and lib.expecto_tfidf_gram_workspace(5, 0) == 0
    assert lib.expecto_tfidf_transform_parts(5, 0, 5) == 0 and lib.expecto_tfidf_transform_workspace(0, 5, 5) == 0
    torch.cuda.synchronize()
    for g in (idf, rs, H, X, out, ws):
        assert g.untouched()


# ---- API -------------------------------------------------------------------------------------

API_CASES = [(37, 3, 200, 12, 11, 8), (130, 2, 200, 16, 12, 16)]


def check_model(model, X, keep, exact, k, what):
    """fit's result against numpy's SVD of the tf-idf matrix, signs equal outright."""
    N = X.shape[0]
    sv_rel, vec = svd_ref.tolerances(exact, N, k)
    sig = exact["singular_values_"][:k]
    err = np.abs(model["singular_values_"] / sig - 1)
    print(f"{what}: singular values rel err {err.max():.3g} (allowed {sv_rel:.3g})")
    assert (err <= sv_rel).all()
    assert model["components_"].dtype == np.float32 and model["components_"].shape == (k, N)
    err = np.abs(model["components_"] - exact["components_"][:k]).max(axis=1)
    print(f"{what}: components err / allowed {np.max(err / vec):.3g}")
    assert (err <= vec).all()
    assert model["x_reduced"].dtype == np.float64 and model["x_reduced"].shape == (len(keep), k)
    err = np.abs(model["x_reduced"] - exact["x_reduced"][:, :k]).max(axis=0)
    print(f"{what}: x_reduced err / allowed {np.max(err / ((vec + sv_rel) * sig)):.3g}")
    assert (err <= (vec + sv_rel) * sig).all()
    evr_tol = 2 * (vec + sv_rel) * sig ** 2 / len(keep) / (exact["explained_variance_"][0] /
                                                           exact["explained_variance_ratio_"][0]) + 1e-15
    assert (np.abs(model["explained_variance_ratio_"] - exact["explained_variance_ratio_"][:k]) <= evr_tol).all()
    assert np.allclose(model["explained_variance_"], np.var(model["x_reduced"], axis=0), rtol=1e-12, atol=0)


@pytest.mark.parametrize("gene_batch", [1, 2])
@pytest.mark.parametrize("marks,files,rows,rank,seed,k", API_CASES)
def test_fit_and_transform(marks, files, rows, rank, seed, k, gene_batch):
    """Several chunks with an uneven last one (3 files by 2) and one file per chunk."""
    from expecto_amd import svd
    X, keep, exact = svd_ref.case(marks, files, rows, rank, seed, k)
    arrays = [X[g * rows:(g + 1) * rows].copy() for g in range(files)]
    model = svd.fit(arrays, keep, n_components=k, gene_batch=gene_batch)
    assert model["rows_per_file"] == rows and len(model["files"]) == files and np.array_equal(model["keep_idx"], keep)
    check_model(model, X, keep, exact, k, f"fit {marks}x{files}x{rows} batch {gene_batch}")
    # the fitted files transformed: x_reduced up to the float32 rounding of components_
    got = svd.transform(model, arrays, gene_batch=gene_batch)
    assert got.dtype == np.float64 and got.shape == (len(keep), k)
    bound = 2.0 ** -23 * svd_ref.row_norms(X, keep)[:, None]
    err = np.abs(got - model["x_reduced"])
    print(f"transform of the fitted files: err / allowed {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    with pytest.raises(ValueError, match="2 rows each"):
        svd.transform(model, [a[:2] for a in arrays])


def test_fit_refusals():
    from expecto_amd import svd
    files = svd_ref.tracks(9, 2, 40, 3, 4)
    with pytest.raises(ValueError, match="exceeds the 9 kept marks"):
        svd.fit(files, np.arange(9), n_components=10)
    bad = [f.copy() for f in files]
    bad[0][:, 4] = 0.0
    bad[1][:, 4] = 0.0
    with pytest.raises(ValueError, match=r"1 kept mark\(s\) have a row sum <= 0 \(first: kept mark 4\)"):
        svd.fit(bad, np.arange(9), n_components=2)
    assert svd.fit(bad, [0, 1, 2, 3, 5, 6, 7, 8], n_components=2)["x_reduced"].shape == (8, 2)   # dropped: fine
    bad = [f.copy() for f in files]
    bad[1][7, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        svd.fit(bad, np.arange(9), n_components=2)
    bad[1][7, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        svd.fit(bad, np.arange(9), n_components=2)
    bad = [f.copy() for f in files]
    bad[0][3, :] = -0.2          # 1 + c_n < 0
    with pytest.raises(ValueError, match=r"1 column\(s\) hold NaN or infinity, or have 1 \+ column sum <= 0"):
        svd.fit(bad, np.arange(9), n_components=2)


# ---- CLI -------------------------------------------------------------------------------------

def run_cli(capsys, argv):
    from expecto_amd import svd
    capsys.readouterr()
    svd.main([str(a) for a in argv])
    return capsys.readouterr().out


def cli_outputs(tmp_path, capsys, flags):
    """fit then transform of the golden inputs; (stdout of both, model, fit's and transform's .npy)."""
    from expecto_amd import svd
    genes = tmp_path / "genes"
    svd_ref.write_golden_inputs(str(genes))
    out_fit = run_cli(capsys, [genes, "--belugaFeatures", FEATURES_TSV, *flags, "-o", tmp_path / "temp_svd",
                               "--gene-batch", 2])
    out_tr = run_cli(capsys, ["transform", genes, tmp_path / "temp_svd" / "svd_100.npz", "--belugaFeatures",
                              FEATURES_TSV, *flags, "-o", tmp_path / "temp_svd_transform", "--gene-batch", 2])
    model = svd.load_model(str(tmp_path / "temp_svd" / "svd_100.npz"))
    assert model["files"] == sorted(svd_ref.golden_names()) and model["rows_per_file"] == svd_ref.GOLDEN_ROWS
    return (out_fit, out_tr, model, np.load(tmp_path / "temp_svd" / "tf_idf_reduced_100.npy"),
            np.load(tmp_path / "temp_svd_transform" / "tf_idf_reduced_100.npy"))


def reduced_bounds(X, keep, exact, k):
    """Allowed |ours - oracle| of x_reduced [1, k] and of the float32 file transform writes [m, k]."""
    sv_rel, vec = svd_ref.tolerances(exact, X.shape[0], k)
    sig = exact["singular_values_"][:k]
    fit_tol = ((vec + sv_rel) * sig)[None, :]
    file_tol = fit_tol + 2.0 ** -23 * svd_ref.row_norms(X, keep)[:, None] + \
        2.0 ** -24 * np.abs(exact["x_reduced"][:, :k])
    return sv_rel, vec, sig, fit_tol, file_tol


def test_cli_golden(tmp_path, capsys):
    """The reference's svd.py + svd_transform.py on the same input with --no_dnase_features: its leading
    16 components within its own distance from the float64 oracle plus our tolerance."""
    X = svd_ref.stack(svd_ref.golden_inputs())
    keep = np.nonzero((pd.read_csv(FEATURES_TSV, sep="\t", index_col=0)["Assay type"] != "DNase").to_numpy())[0]
    exact = svd_ref.fit_exact(X, keep, 100)
    z = np.load(os.path.join(GOLD, "leading.npz"))
    out_fit, out_tr, model, red_fit, red_tr = cli_outputs(tmp_path, capsys, ["--no_dnase_features"])
    assert out_fit == open(os.path.join(GOLD, "stdout_svd.txt")).read()
    assert out_tr == open(os.path.join(GOLD, "stdout_transform.txt")).read()
    for red in (red_fit, red_tr):
        assert str(red.dtype) == str(z["reduced_dtype"]) == "float32"
        assert red.shape == tuple(z["reduced_shape"]) == (1668, 100)
    sv_rel, vec, sig, fit_tol, file_tol = reduced_bounds(X, keep, exact, LEADING)
    oracle = exact["x_reduced"][:, :LEADING]
    gold = z["tf_idf_reduced"].astype(np.float64)
    for red in (red_fit, red_tr):
        assert (np.abs(red[:, :LEADING] - gold) <= np.abs(oracle - gold) + file_tol).all()
    order = open(os.path.join(GOLD, "files.txt")).read().split()
    gold = z["components"].reshape(LEADING, len(order), svd_ref.GOLDEN_ROWS)[:, np.argsort(order)].reshape(LEADING, -1)
    assert (np.abs(model["components_"][:LEADING] - gold) <=
            np.abs(exact["components_"][:LEADING] - gold) + vec[:, None]).all()
    gold = z["singular_values"][:LEADING].astype(np.float64)
    assert (np.abs(model["singular_values_"][:LEADING] - gold) <= np.abs(sig - gold) + sv_rel * sig).all()
    gold = z["explained_variance_ratio"][:LEADING].astype(np.float64)
    want = exact["explained_variance_ratio_"][:LEADING]
    full_var = exact["explained_variance_"][0] / exact["explained_variance_ratio_"][0]
    evr_tol = 2 * (vec + sv_rel) * sig ** 2 / len(keep) / full_var + 1e-15
    assert (np.abs(model["explained_variance_ratio_"][:LEADING] - gold) <= np.abs(want - gold) + evr_tol).all()
    # all 100 components against the oracle
    check_model(model, X, keep, exact, 100, "golden input, no DNase")


def test_cli_transform_of_a_sklearn_dump(tmp_path, capsys):
    """A TruncatedSVD joblib dump whose columns follow another file order than the sorted one (as the
    reference's glob order does): refused without --file-order, and with it the files are read in
    the dump's order and the result is the fit's x_reduced."""
    joblib = pytest.importorskip("joblib")
    decomposition = pytest.importorskip("sklearn.decomposition")
    from expecto_amd import svd
    marks, files, rows, rank, seed, k = API_CASES[0]
    X, keep, exact = svd_ref.case(marks, files, rows, rank, seed, k)
    genes = tmp_path / "genes"
    genes.mkdir()
    names = ["a.npy", "b.npy", "c.npy"]
    for g, name in enumerate(names):
        np.save(genes / name, X[g * rows:(g + 1) * rows])
    feat = tmp_path / "features.tsv"
    with open(FEATURES_TSV) as src, open(feat, "w") as f:
        f.writelines(src.readlines()[:1 + marks])
    run_cli(capsys, [genes, "--belugaFeatures", feat, "-o", tmp_path / "fit", "--n_components", k, "--gene-batch", 2])
    model = svd.load_model(str(tmp_path / "fit" / f"svd_{k}.npz"))
    assert model["files"] == names
    order = ["c.npy", "a.npy", "b.npy"]
    est = decomposition.TruncatedSVD(n_components=k)
    est.components_ = np.ascontiguousarray(
        model["components_"].reshape(k, files, rows)[:, [names.index(s) for s in order]].reshape(k, -1))
    joblib.dump(est, tmp_path / "svd.joblib")
    argv = ["transform", genes, tmp_path / "svd.joblib", "--belugaFeatures", feat, "-o", tmp_path / "tr", "--gene-batch", 2]
    with pytest.raises(ValueError, match="does not record the order of the files"):
        run_cli(capsys, argv)
    (tmp_path / "order.txt").write_text("".join(s + "\n" for s in order))
    run_cli(capsys, argv + ["--file-order", tmp_path / "order.txt"])
    got = np.load(tmp_path / "tr" / f"tf_idf_reduced_{k}.npy")
    assert got.dtype == np.float32 and got.shape == (marks, k)
    bound = 2.0 ** -23 * svd_ref.row_norms(X, keep)[:, None] + 2.0 ** -24 * np.abs(model["x_reduced"])
    assert (np.abs(got - model["x_reduced"]) <= bound).all()
    # the same dump paired with the files in sorted order is what the list prevents: far outside
    (tmp_path / "order.txt").write_text("".join(s + "\n" for s in names))
    run_cli(capsys, argv + ["--file-order", tmp_path / "order.txt"])
    wrong = np.load(tmp_path / "tr" / f"tf_idf_reduced_{k}.npy")
    assert (np.abs(wrong - model["x_reduced"]) > 100 * bound).any()


def test_cli_without_ablation(tmp_path, capsys):
    """No ablation flag (2002 marks): the case the reference scripts crash on, against the oracle."""
    X = svd_ref.stack(svd_ref.golden_inputs())
    keep = np.arange(svd_ref.GOLDEN_MARKS)
    exact = svd_ref.fit_exact(X, keep, 100)
    out_fit, out_tr, model, red_fit, red_tr = cli_outputs(tmp_path, capsys, [])
    assert out_fit == out_tr == "Number of features included in model: 2002\nTracks shape: (2002, 600)\n"
    check_model(model, X, keep, exact, 100, "golden input, all marks")
    _, _, _, _, file_tol = reduced_bounds(X, keep, exact, 100)
    for red in (red_fit, red_tr):
        assert red.dtype == np.float32 and red.shape == (2002, 100)
        assert (np.abs(red - exact["x_reduced"]) <= file_tol).all()
