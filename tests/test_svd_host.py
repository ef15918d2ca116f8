"""CPU: the oracle of the tf-idf SVD tests (tests/svd_ref.py) anchored against numpy's SVD and the
reference's golden run, and the host side of expecto_amd.svd (parsers, model files, refusals)."""
import os

import numpy as np
import pandas as pd
import pytest

import svd_ref
from conftest import GOLDEN

GOLD = os.path.join(GOLDEN, "svd")
FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
LEADING = 16
# (marks, files, rows, rank, seed, k): the shapes test_gpu_svd.py runs the API on
API_CASES = [(37, 3, 200, 12, 11, 8), (130, 2, 200, 16, 12, 16)]


def no_dnase_keep():
    df = pd.read_csv(FEATURES_TSV, sep="\t", index_col=0)
    return np.nonzero((df["Assay type"] != "DNase").to_numpy())[0]


@pytest.fixture(scope="module")
def golden_case():
    X = svd_ref.stack(svd_ref.golden_inputs())
    keep = no_dnase_keep()
    return X, keep, svd_ref.fit_exact(X, keep, 100)


def check_gram_route(X, keep, exact, k):
    N = X.shape[0]
    got = svd_ref.fit_gram(X, keep, k)
    sv_rel, vec = svd_ref.tolerances(exact, N, k)
    sig = exact["singular_values_"][:k]
    assert (np.abs(got["singular_values_"] / sig - 1) <= sv_rel).all()
    assert (np.abs(got["components_"] - exact["components_"][:k]) <= vec[:, None]).all()
    assert (np.abs(got["x_reduced"] - exact["x_reduced"][:, :k]) <= ((vec + sv_rel) * sig)[None, :]).all()
    assert np.allclose(got["explained_variance_ratio_"], exact["explained_variance_ratio_"][:k], rtol=1e-9, atol=1e-15)


@pytest.mark.parametrize("marks,files,rows,rank,seed,k", API_CASES)
def test_gram_route_equals_exact_svd(marks, files, rows, rank, seed, k):
    X, keep, exact = svd_ref.case(marks, files, rows, rank, seed, k)
    check_gram_route(X, keep, exact, k)


def test_gram_route_equals_exact_svd_golden(golden_case):
    X, keep, exact = golden_case
    check_gram_route(X, keep, exact, LEADING)
    check_gram_route(X, np.arange(svd_ref.GOLDEN_MARKS), svd_ref.fit_exact(X, np.arange(svd_ref.GOLDEN_MARKS), LEADING),
                     LEADING)


def test_full_variance_identity():
    from expecto_amd import svd
    X, keep, _ = svd_ref.case(*API_CASES[0])
    A = svd_ref.tfidf(X, keep)
    G = A @ A.T
    want = np.var(A, axis=0).sum()
    assert abs(svd.full_variance(G) - want) <= 1e-13 * want
    assert abs(G.trace() / len(keep) - G.sum() / len(keep) ** 2 - want) <= 1e-13 * want


def test_sign_rule():
    from expecto_amd import svd
    V = np.array([[0.1, -0.7, 0.7, 0.2], [0.5, 0.5, -0.5, 0.1], [-0.3, 0.2, 0.1, 0.0], [0.0, 0.0, 0.0, 0.0]])
    want = np.array([-1.0, 1.0, -1.0, 1.0])      # ties go to the first entry; a zero row keeps its sign
    assert np.array_equal(svd_ref.flip(V), want)
    assert np.array_equal(svd.sign_flip(V), want)
    assert np.array_equal(svd.sign_flip(V.astype(np.float32)), want)


def test_golden_signs_are_unambiguous(golden_case):
    """The largest |entry| of each of the 16 leading components beats the runner-up by >= 1e-3 of
    itself, four orders above float32 rounding, with and without the ablation."""
    X, keep, exact = golden_case
    full = svd_ref.fit_exact(X, np.arange(svd_ref.GOLDEN_MARKS), LEADING)
    for comps in (exact["components_"][:LEADING], full["components_"]):
        top = np.sort(np.abs(comps), axis=1)
        margin = (top[:, -1] - top[:, -2]) / top[:, -1]
        assert margin.min() >= 1e-3, margin


def golden_components_sorted(z):
    """The golden components' columns moved from the reference's glob order to sorted file order."""
    order = open(os.path.join(GOLD, "files.txt")).read().split()
    assert sorted(order) == sorted(svd_ref.golden_names())
    blocks = z["components"].reshape(LEADING, len(order), svd_ref.GOLDEN_ROWS)
    return blocks[:, np.argsort(order)].reshape(LEADING, -1)


def test_oracle_equals_reference_leading_components(golden_case):
    """The reference's own error on its leading 16 components: float32 sums of up to 1668 terms, so
    at most 1668 * 2^-24 = 1e-4 of the largest entry (measured: about 1e-6)."""
    X, keep, exact = golden_case
    z = np.load(os.path.join(GOLD, "leading.npz"))
    assert str(z["reduced_dtype"]) == "float32" and tuple(z["reduced_shape"]) == (len(keep), 100)
    rel = len(keep) * 2.0 ** -24
    for got, want in ((z["tf_idf_reduced"], exact["x_reduced"][:, :LEADING]),
                      (golden_components_sorted(z), exact["components_"][:LEADING]),
                      (z["singular_values"][:LEADING], exact["singular_values_"][:LEADING]),
                      (z["explained_variance_ratio"][:LEADING], exact["explained_variance_ratio_"][:LEADING])):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= rel * np.abs(want).max()
    assert open(os.path.join(GOLD, "stdout_svd.txt")).read().endswith("Tracks shape: (1668, 600)\n")


# ---- expecto_amd.svd, host side ----------------------------------------------------------------

def test_parsers():
    from expecto_amd import svd
    a = svd.build_parser().parse_args(["dir", "--belugaFeatures", "f.tsv"])
    assert (a.replicate_expecto_features_dir, a.out_dir, a.n_components, a.gene_batch) == ("dir", "temp_svd", 100, 256)
    assert not (a.no_tf_features or a.no_dnase_features or a.no_histone_features or a.intersect_with_lambert or a.no_pol2)
    a = svd.build_parser().parse_args(["dir", "--belugaFeatures", "f.tsv", "--no_dnase_features", "--no_pol2", "-o", "x",
                                       "--n_components", "20", "--gene-batch", "4"])
    assert a.no_dnase_features and a.no_pol2 and (a.out_dir, a.n_components, a.gene_batch) == ("x", 20, 4)
    t = svd.build_transform_parser().parse_args(["dir", "m.npz", "--belugaFeatures", "f.tsv", "--no_tf_features"])
    assert (t.svd_joblib, t.out_dir, t.no_tf_features) == ("m.npz", "temp_svd_transform", True)


def toy_model(k=3, files=2, rows=5, marks=7):
    rng = np.random.default_rng(5)
    return {"components_": rng.normal(size=(k, files * rows)).astype(np.float32), "singular_values_": rng.random(k),
            "explained_variance_": rng.random(k), "explained_variance_ratio_": rng.random(k),
            "x_reduced": rng.normal(size=(marks - 2, k)), "files": [f"g{i}.npy" for i in range(files)],
            "keep_idx": np.arange(marks - 2), "rows_per_file": rows}


def test_model_round_trip(tmp_path):
    from expecto_amd import svd
    model = toy_model()
    svd.save_model(str(tmp_path / "svd_3.npz"), model)
    back = svd.load_model(str(tmp_path / "svd_3.npz"))
    assert set(back) == set(svd.MODEL_KEYS)
    assert back["files"] == model["files"] and back["rows_per_file"] == 5
    for key in ("components_", "singular_values_", "explained_variance_", "explained_variance_ratio_", "x_reduced",
                "keep_idx"):
        assert back[key].dtype == np.asarray(model[key]).dtype and np.array_equal(back[key], model[key])


def test_transform_refuses_other_files(tmp_path):
    """Checked on the host, before any device call."""
    from expecto_amd import svd
    model = toy_model()

    def write(names, rows=5):
        d = tmp_path / f"d{len(os.listdir(tmp_path))}"
        d.mkdir()
        for name in names:
            np.save(d / name, np.ones((rows, 7), np.float32))
        return [str(d / name) for name in names]

    with pytest.raises(ValueError, match="3 files given, the model was fitted on 2"):
        svd.transform(model, write(["g0.npy", "g1.npy", "g2.npy"]))
    with pytest.raises(ValueError, match=r"file 1 is g9.npy, the model was fitted on g1.npy there \(basenames differ\)"):
        svd.transform(model, write(["g0.npy", "g9.npy"]))
    with pytest.raises(ValueError, match="4 rows each, the model was fitted on 5 rows per file"):
        svd.transform(model, write(["g0.npy", "g1.npy"], rows=4))
    with pytest.raises(ValueError, match="no input files"):
        svd.transform(model, [])


def test_sklearn_dump_needs_the_file_order(tmp_path):
    """A reference dump's columns follow its glob order, which it does not record: refused without the
    list of basenames, and with it the model carries that order."""
    joblib = pytest.importorskip("joblib")
    decomposition = pytest.importorskip("sklearn.decomposition")
    from expecto_amd import svd
    A = np.random.default_rng(2).random((7, 12)).astype(np.float32)
    est = decomposition.TruncatedSVD(n_components=3, random_state=1).fit(A)
    path = str(tmp_path / "svd_3.joblib")
    joblib.dump(est, path)
    with pytest.raises(ValueError, match="does not record the order of the files"):
        svd.load_model(path, keep_idx=np.arange(7))
    with pytest.raises(ValueError, match="does not record the kept marks"):
        svd.load_model(path, file_order=["b.npy", "a.npy"])
    model = svd.load_model(path, keep_idx=np.arange(7), file_order=["b.npy", "a.npy"])
    assert model["files"] == ["b.npy", "a.npy"] and model["components_"].dtype == np.float32
    assert np.array_equal(model["components_"], est.components_)
    t = svd.build_transform_parser().parse_args(["dir", path, "--belugaFeatures", "f.tsv", "--file-order", "o.txt"])
    assert t.file_order == "o.txt"


def test_fit_refuses_bad_requests_on_the_host():
    from expecto_amd import svd
    files = svd_ref.tracks(9, 2, 4, 2, 1)
    with pytest.raises(ValueError, match="exceeds the 5 kept marks"):
        svd.fit(files, np.arange(5), n_components=6)
    with pytest.raises(ValueError, match="or the 8 columns"):
        svd.fit(files, np.arange(9), n_components=9)
    with pytest.raises(ValueError, match="distinct"):
        svd.fit(files, [1, 1, 2], n_components=1)
    with pytest.raises(ValueError, match=r"\[0, 9\)"):
        svd.fit(files, [1, 9], n_components=1)
    with pytest.raises(ValueError, match="has shape"):
        svd.fit([files[0], files[1][:3]], np.arange(9), n_components=1)


def test_eig_top_refuses_unresolved_components():
    from expecto_amd import svd
    m = 6
    Q = np.linalg.qr(np.random.default_rng(3).normal(size=(m, m)))[0]
    lam = np.array([1.0, 0.5, 1e-3, 1e-10, 1e-11, 0.0])
    G = (Q * lam) @ Q.T
    got, vec = svd.eig_top(G, 3)
    assert np.allclose(got, lam[:3], rtol=1e-12) and vec.shape == (m, 3)
    with pytest.raises(ValueError, match="2 of the 5 requested components"):
        svd.eig_top(G, 5)
