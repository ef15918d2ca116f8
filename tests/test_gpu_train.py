"""GPU: gblinear training (expecto_gblinear_train_round / _predict_cols / _rmse,
xgblinear.train, the train CLI) against the numpy restatements of tests/gblinear_ref.py.

The bar is derived, not chosen: noise = max|R32 - R64| over [w; b] is the size of the float32
rounding in the steps themselves, and the GPU result (the same steps, its double sums in another
order) must lie within it: max|GPU - R32| <= noise.  The share of weights bit-equal to R32 is
printed for information (a one-ulp flip of a dw is legitimate)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gblinear_ref import make_problem, noise_of, train_ref

pytestmark = pytest.mark.gpu


def _wb(models):
    ms = models if isinstance(models, list) else [models]
    return np.stack([np.concatenate([m.weights[:, 0], m.bias]) for m in ms]).astype(np.float64)


def _check(models, r32, noise, what):
    got = _wb(models)
    err = np.abs(got - r32).max(1)
    same = (got.astype(np.float32) == r32.astype(np.float32)).mean()
    print(f"{what}: max|GPU - R32| {err.max():.3g}, noise {noise.min():.3g}, bit-equal share {same:.4f}")
    assert np.isfinite(got).all()
    assert (err <= noise).all(), (what, err, noise)


@pytest.fixture(scope="module")
def case1():
    return make_problem(1003, 97, seed=11)


@pytest.mark.parametrize("eta,lam,rounds", [(0.01, 100.0, 5), (0.5, 1.0, 8), (1.0, 0.0, 3)])
def test_case1_odd_rows(case1, eta, lam, rounds):
    from expecto_amd.xgblinear import train
    X, y, h = case1
    r32, noise, h32 = noise_of(X, y, h, eta=eta, lam=lam, rounds=rounds)
    m, hist = train(X, y[0], h[0], num_round=rounds, eta=eta, lambda_=lam)
    _check(m, r32, noise, f"n=1003 F=97 eta={eta} lambda={lam}")
    assert hist.shape == (rounds, 1)
    np.testing.assert_allclose(hist[:, 0], h32[0, :, 0], rtol=1e-5)


@pytest.mark.parametrize("n,F", [(37, 1), (1, 3)])
def test_case2_less_than_a_wave(n, F):
    from expecto_amd.xgblinear import train
    X, y, h = make_problem(n, F, seed=3)
    h = np.maximum(h, 1.0)                      # a single row of weight 0 has no bias step (0 / 0)
    r32, noise, _ = noise_of(X, y, h, eta=0.5, lam=1.0, rounds=4)
    m, _ = train(X, y[0], h[0], num_round=4, eta=0.5, lambda_=1.0)
    _check(m, r32, noise, f"n={n} F={F}")


def test_case3_row_cap():
    from expecto_amd import xgblinear
    cap = xgblinear.TRAIN_MAX_ROWS
    assert cap >= 24576
    X, y, h = make_problem(cap + 1, 8, seed=4)
    r32, noise, _ = noise_of(X[:cap], y[:, :cap], h[:, :cap], eta=0.5, lam=1.0, rounds=2)
    m, _ = xgblinear.train(X[:cap], y[0, :cap], h[0, :cap], num_round=2, eta=0.5, lambda_=1.0)
    _check(m, r32, noise, f"n={cap} F=8")
    with pytest.raises(RuntimeError, match=str(cap)):
        xgblinear.train(X, y[0], h[0], num_round=2, eta=0.5, lambda_=1.0)


def test_case3_over_the_cap_launches_nothing():
    import torch
    from expecto_amd import _lib, xgblinear
    lib = _lib.load()
    n, F = xgblinear.TRAIN_MAX_ROWS + 1, 2
    X = torch.ones(F, n, device="cuda")
    y = torch.ones(n, device="cuda")
    w = torch.full((F + 1,), 7.0, device="cuda")
    sh = torch.zeros(F, dtype=torch.float64, device="cuda")
    st = lib.expecto_gblinear_train_round(_lib.dptr(X), n, n, F, 1, _lib.dptr(y), 0, None, 0, _lib.dptr(w),
                                          _lib.dptr(sh), 1, 0.5, 1.0, 0.0, 0.0, 2.0, None, _lib.stream_ptr())
    assert st == -1 and b"24576" in lib.expecto_last_error()
    torch.cuda.synchronize()
    assert (w.cpu() == 7.0).all()
    assert lib.expecto_gblinear_train_round(None, 0, 0, F, 1, None, 0, None, 0, None, None, 1, 0.5, 1.0, 0.0, 0.0,
                                            2.0, None, None) == 0
    assert lib.expecto_gblinear_train_round(None, 8, 8, F, 1, None, 0, None, 0, None, None, 1, 0.5, 1.0, 0.0, 0.0,
                                            2.0, None, None) == -1
    assert b"null" in lib.expecto_last_error()
    assert lib.expecto_gblinear_predict_cols(None, 8, 8, F, 1, None, 2.0, None, None) == -1
    assert lib.expecto_gblinear_rmse(None, None, 0, None, 0, 8, 0, None, None) == 0


def test_case4_l1_clips_weights_to_zero(case1):
    from expecto_amd.xgblinear import train
    X, y, h = case1
    r32, noise, _ = noise_of(X, y, h, eta=0.5, lam=1.0, alpha=50.0, rounds=6)
    zero = r32[0, :-1] == 0.0
    assert zero.sum() >= 1                      # the -w clip is exercised
    m, _ = train(X, y[0], h[0], num_round=6, eta=0.5, lambda_=1.0, alpha=50.0)
    _check(m, r32, noise, "alpha=50")
    print("weights at exactly 0:", int(zero.sum()), "of", zero.size)
    assert (m.weights[zero, 0] == 0.0).all()


def test_case5_flat_columns_stay_zero(case1):
    from expecto_amd.xgblinear import train
    X, y, h = case1
    X = X.copy()
    X[:, 5] = 0.0
    X[:, 40] = 1e-4
    h = np.minimum(h, 1.0)                      # weights 0 / 1 here: sh = 1e-8 * sum h must stay below 1e-5
    assert float(h.sum()) * 1e-8 < 0.9e-5
    r32, noise, _ = noise_of(X, y, h, eta=0.5, lam=1.0, rounds=4)
    assert r32[0, 5] == 0.0 and r32[0, 40] == 0.0
    m, _ = train(X, y[0], h[0], num_round=4, eta=0.5, lambda_=1.0)
    _check(m, r32, noise, "flat columns")
    assert m.weights[5, 0] == 0.0 and m.weights[40, 0] == 0.0


def test_case6_batch_invariance():
    from expecto_amd.xgblinear import ColMatrix, train
    X, y, h = make_problem(1003, 33, seed=6, B=5)
    Xc = ColMatrix(X)
    kw = dict(num_round=4, eta=0.5, lambda_=1.0)
    ms, hist = train(Xc, y, h, **kw)
    ms2, hist2 = train(Xc, y, h, **kw)
    assert _wb(ms).tobytes() == _wb(ms2).tobytes() and hist.tobytes() == hist2.tobytes()
    assert hist.shape == (5, 4, 1)
    for b in range(5):
        m1, h1 = train(Xc, y[b], h[b], **kw)
        assert _wb(m1).tobytes() == _wb(ms[b]).tobytes(), b
        assert h1.tobytes() == hist[b].tobytes(), b
    r32, noise, _ = noise_of(X, y, h, eta=0.5, lam=1.0, rounds=4)
    _check(ms, r32, noise, "batch of 5")


def test_case7_bootstrap_by_weights(case1):
    from expecto_amd.xgblinear import train
    X, y, h = case1
    kw = dict(num_round=4, eta=0.5, lambda_=1.0)
    r32, noise, _ = noise_of(X, y, h, eta=0.5, lam=1.0, rounds=4)
    by_weight, _ = train(X, y[0], h[0], **kw)
    idx = np.repeat(np.arange(X.shape[0]), h[0].astype(int))          # the rows, physically duplicated
    dup, _ = train(X[idx], y[0, idx], None, **kw)
    keep = h[0] > 0                                                   # zero-weight rows removed
    cut, _ = train(X[keep], y[0, keep], h[0, keep], **kw)
    for other, what in ((dup, "duplicated rows"), (cut, "rows removed")):
        err = np.abs(_wb(by_weight) - _wb(other)).max()
        print(f"weights vs {what}: {err:.3g} (noise {noise[0]:.3g})")
        assert err <= noise[0]
    _check(by_weight, r32, noise, "bootstrap weights")


def test_case8_predictions_match_the_scoring_kernel(case1):
    import torch
    from expecto_amd.xgblinear import ColMatrix, predict_cols, train
    X, y, h = case1
    Xc = ColMatrix(X)
    m, hist = train(Xc, y[0], h[0], num_round=5, eta=0.5, lambda_=1.0)
    p = predict_cols(Xc, m)
    q = m.predict(torch.from_numpy(X.astype(np.float64)).cuda())
    assert torch.equal(p, q)
    p = p.cpu().numpy()
    d = y[0] - p
    want = np.sqrt(((d * d) * h[0]).astype(np.float64).sum() / h[0].astype(np.float64).sum())
    assert abs(hist[-1, 0] - want) <= 1e-6 * want


def test_case9_cli_end_to_end(tmp_path, capsys):
    import pandas as pd
    from expecto_amd import train as cli
    from expecto_amd.predict import get_keep_mask
    from expecto_amd.xgblinear import GBLinear

    rng = np.random.default_rng(9)
    G = 300
    X = rng.standard_normal((G, 20020)) * rng.uniform(0.01, 3.0, 20020)
    np.save(tmp_path / "X.npy", X)
    chrom = ["chr1", "chr2", "chr8", "chr3", "chrX", "chr4", "chr8", "chrY"]
    anno = pd.DataFrame({"id": [f"G{i}" for i in range(G)], "seqnames": [chrom[i % 8] for i in range(G)],
                         "type": ["rRNA" if i % 10 == 9 else "protein_coding" for i in range(G)]})
    anno.to_csv(tmp_path / "geneanno.csv", index=False)
    exp = pd.DataFrame({"id": anno["id"], "tA": rng.uniform(0.1, 50, G), "tB": rng.uniform(0.1, 50, G)})
    exp.to_csv(tmp_path / "exp.csv", index=False)
    feats = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
    out = tmp_path / "models"
    args = cli.build_parser().parse_args(
        ["--expFile", str(tmp_path / "exp.csv"), "--inputFile", str(tmp_path / "X.npy"), "--annoFile",
         str(tmp_path / "geneanno.csv"), "--belugaFeatures", feats, "--num_round", "3", "--no_tf_features",
         "--targetIndex", "1", "2", "--n_bootstrap", "2", "--output_dir", str(out)])
    capsys.readouterr()
    res = cli.run(args)
    text = capsys.readouterr().out
    assert [(r["name"], r["boot"]) for r in res] == [("tA", 0), ("tA", 1), ("tB", 0), ("tB", 1)]

    df = pd.read_csv(feats, sep="\t", index_col=0)
    keep = np.nonzero(np.asarray(df["Assay type"] != "TF"))[0]
    i = np.arange(G)
    tr = np.isin(i % 8, [0, 1, 3, 5]) & (i % 10 != 9)
    te = np.isin(i % 8, [2, 6]) & (i % 10 != 9)
    Xs = X.reshape(G, 10, 2002)[:, :, keep].reshape(G, -1)
    ylog = np.log(exp[["tA", "tB"]].to_numpy().T + 0.0001)
    ys = np.repeat(ylog, 2, axis=0)                                  # tA, tA, tB, tB
    hs = np.stack([cli.bootstrap_weights(tr, k)[tr] for k in (0, 1)] * 2)
    r32, noise, h32 = noise_of(Xs[tr], ys[:, tr], hs, eta=0.01, lam=100.0, rounds=3,
                               evals=[(Xs[te], ys[:, te], None)])
    lines = [l for l in text.splitlines() if l.startswith("[")]
    assert len(lines) == 12
    for m, r in enumerate(res):
        stem = f"{out}/expecto_all.pseudocount0.0001.lambda100.round3.basescore2.{r['name']}.boot{r['boot']}"
        assert r["save"] == stem + ".save" and os.path.exists(stem + ".save") and os.path.exists(stem + ".dump")
        back = GBLinear.load(stem + ".save")
        assert back.num_feature == 10 * len(keep) and back.base_score == 2.0
        _check(back, r32[m:m + 1], noise[m:m + 1], f"CLI model {r['name']} boot {r['boot']}")
        assert GBLinear.load(stem + ".dump", base_score=2.0).num_feature == 10 * len(keep)
        for k in range(3):
            assert lines[3 * m + k] == "[%d]\teval-rmse:%f\ttrain-rmse:%f" % (k, r["history"][k, 1],
                                                                              r["history"][k, 0])
        np.testing.assert_allclose(r["history"], h32[m], rtol=1e-5)
    assert text.count("SignificanceResult") + text.count("SpearmanrResult") == 4
