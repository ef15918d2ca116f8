"""GPU: per-model hyper-parameters in the gblinear round kernel and cross-validation on top of them
(expecto_gblinear_train_round_hp, xgblinear.train with sequences, xgblinear.cv, train --cv).

The kernel tests compare bits (``assert_bits``), like tests/test_gpu_train_kernels.py, whose
buffers they use: outputs in pattern-guarded buffers, X / y / h between NaN margins.  Model m of a
batch with a row of (eta, lambda, alpha, lambda_bias) each must equal, after every one of three
rounds, both the scalar entry point run on model m alone with those four numbers and
oracle/gblinear_train_np.py called with them.  The layers above are held to each other in bits
(a batch to its models alone, any chunk to any other, cv's rmse to single ``train`` calls) and,
where the sums run in another order (zero weights against removed rows), to
``noise = max|R32 - R64|`` of the numpy restatements of tests/gblinear_ref.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gblinear_ref import make_problem, noise_of
from guarded import ST, Guarded, assert_bits
from test_gpu_train_kernels import _batch, _matrix, _problem, _ptr, last_error

from oracle import gblinear_train_np as tree

pytestmark = pytest.mark.gpu

BASE = 2.0
# eta, lambda, alpha, lambda_bias
HYPER5 = np.array([[0.5, 1.0, 0.0, 0.0],
                   [0.5, 1.0, 50.0, 0.0],        # alpha clips weights to exact zeros
                   [1.0, 0.0, 0.0, 0.0],         # lambda 0: a flat column has sh = 0 < 1e-5 and only the zero branch
                   [0.3, 2.0, 0.5, 0.75],        # lambda_bias > 0
                   [0.01, 100.0, 0.0, 0.0]])     # the paper's constants


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


class _Doubles:
    """A float64 table on the device between NaN margins: a row read off by one poisons a model."""

    def __init__(self, a, margin=64):
        import torch
        a = np.ascontiguousarray(a, np.float64)
        host = np.full(margin + a.size + margin, np.nan)
        host[margin:margin + a.size] = a.reshape(-1)
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin


def run_hp(lib, X, y, h, hyper, rounds=3, compare_oracle=None):
    """Three rounds of the batch through expecto_gblinear_train_round_hp; after every round w, sh
    and pred of every model m in ``compare_oracle`` (default: all) must equal the scalar entry
    point run on m alone (n_models = 1, pointers at model m) and the oracle run on m alone, both
    with row m of ``hyper`` as scalars.  Returns the oracle's last w and sh and the device's last w."""
    n, F = X.shape
    B = hyper.shape[0]
    models = range(B) if compare_oracle is None else compare_oracle
    Xd, yd, hd, hyd = _matrix(X, n), _batch(y, B, n), _batch(h, B, n), _Doubles(hyper)
    zeros = np.zeros((B, F + 1), np.float32)
    wd, wa = Guarded((B, F + 1), np.float32).put(zeros), Guarded((B, F + 1), np.float32).put(zeros)
    shd, sha = (Guarded((B, F), np.float64), Guarded((B, F), np.float64)) if F else (None, None)
    w, sh = zeros.copy(), np.zeros((B, F))
    for r in range(rounds):
        predd, preda = (Guarded((B, n), np.float32), Guarded((B, n), np.float32)) if r else (None, None)
        st = lib.expecto_gblinear_train_round_hp(_ptr(Xd), n, n, F, B, yd.ptr, n, hd.ptr, n, wd.ptr, _ptr(shd),
                                                 int(r == 0), hyd.ptr, BASE, _ptr(predd), ST())
        assert st == 0, last_error(lib)
        for m in range(B):
            st = lib.expecto_gblinear_train_round(
                _ptr(Xd), n, n, F, 1, yd.ptr + 4 * m * n, n, hd.ptr + 4 * m * n, n, wa.ptr + 4 * m * (F + 1),
                sha.ptr + 8 * m * F if F else None, int(r == 0), *(float(v) for v in hyper[m]), BASE,
                preda.ptr + 4 * m * n if r else None, ST())
            assert st == 0, last_error(lib)
        tag = f"n {n} F {F} B {B} round {r}"
        got_w, got_sh, got_pred = wd.result(), shd.result() if F else None, predd.result() if r else None
        assert_bits(got_w, wa.result(), f"w: per-model table against scalars alone, {tag}")
        if F:
            assert_bits(got_sh, sha.result(), f"sh: per-model table against scalars alone, {tag}")
        if r:
            assert_bits(got_pred, preda.result(), f"pred: per-model table against scalars alone, {tag}")
        for m in models:
            wm, shm, pm = tree.train_round(X, y[m], h[m], w[m], None if r == 0 else sh[m], r == 0,
                                           *(float(v) for v in hyper[m]), BASE)
            w[m], sh[m] = wm[0], shm[0]
            assert_bits(got_w[m], w[m], f"w of model {m} against the oracle, {tag}")
            if F:
                assert_bits(got_sh[m], sh[m], f"sh of model {m} against the oracle, {tag}")
            if r:
                assert_bits(got_pred[m], pm[0], f"pred of model {m} against the oracle, {tag}")
    return w, sh, got_w


# ---- expecto_gblinear_train_round_hp -------------------------------------------------------

@pytest.mark.parametrize("F", [0, 1, 2, 5])
@pytest.mark.parametrize("n", [1, 1023, 1025, 2049])
def test_round_hp_five_models(lib, n, F):
    """n: one row, the last lane of row slot 0, one and 1,025 rows into slot 1.  F: the two-column
    pipeline's empty, odd and even tails.  With F >= 2 the last column is flat (all zeros)."""
    X, y, h = _problem(n, F, seed=5000 + 10 * n + F, B=5)
    if F >= 2:
        X[:, F - 1] = 0.0
    w, sh, _ = run_hp(lib, X, y, h, HYPER5)
    assert len({w[m].tobytes() for m in range(5)}) == 5
    if F >= 2:
        assert (sh[:, F - 1] == 0).all() and (w[:, F - 1] == 0).all()        # lambda = 0 included: the zero branch
    if F == 5 and n >= 1023:
        assert (w[[0, 2, 4], :F - 1] != 0).all() and np.isfinite(w).all()
        assert (w[3, F] != w[0, F]) and (w[3, F] != 0)


def test_round_hp_l1_model_has_exact_zeros(lib):
    """The alpha = 50 row of the table clips some of its model's weights to +0.0 and moves others;
    its neighbours, without alpha, keep every weight away from zero."""
    X, y, h = _problem(1025, 12, seed=11, B=5)
    w, _, _ = run_hp(lib, X, y, h, HYPER5)
    zero = w[:, :-1] == 0
    assert zero[1].any() and (~zero[1]).any() and not np.signbit(w[1, :-1][zero[1]]).any()
    assert not zero[[0, 2, 4]].any()


def test_round_hp_more_workgroups_than_cus(lib):
    X, y, h = _problem(64, 3, seed=5100, B=257)
    hyper = HYPER5[np.arange(257) % 5]
    w, _, _ = run_hp(lib, X, y, h, hyper)
    assert len({w[m].tobytes() for m in range(257)}) == 257


def test_round_hp_nan_lambda_leaves_its_neighbours_alone(lib):
    """The C entry point does not validate: a NaN lambda gives the middle model whatever the
    arithmetic gives (the same as the scalar entry point with NaN, compared inside run_hp), and the
    models around it keep the bits they have alone and in the oracle."""
    X, y, h = _problem(1025, 4, seed=5200, B=3)
    hyper = HYPER5[[0, 1, 3]].copy()
    hyper[1, 1] = np.nan
    w, _, got = run_hp(lib, X, y, h, hyper, compare_oracle=[0, 2])
    assert np.isfinite(got[[0, 2]]).all() and (got[[0, 2], :-1] != 0).any()
    assert_bits(got[[0, 2]], w[[0, 2]], "neighbours of the NaN model")


def test_round_hp_refusals_write_nothing(lib):
    n, F, B = 70, 3, 2
    X, y, h = _problem(n, F, seed=5300, B=B)
    Xd, yd, hd, hyd = _matrix(X, n), _batch(y, B, n), _batch(h, B, n), _Doubles(HYPER5[:B])
    w, sh, pred = Guarded((B, F + 1), np.float32), Guarded((B, F), np.float64), Guarded((B, n), np.float32)

    def call(ld=n, n=n, F=F, B=B, w=w.ptr, hyper=hyd.ptr):
        return lib.expecto_gblinear_train_round_hp(Xd.ptr, ld, n, F, B, yd.ptr, n, hd.ptr, n, w, sh.ptr, 1, hyper,
                                                   BASE, pred.ptr, ST())

    assert call(hyper=None) == -1 and "null" in last_error(lib)
    assert call(ld=n - 1) == -1 and "ld >= n" in last_error(lib)
    assert call(n=24577, ld=24577) == -1 and "24576" in last_error(lib)
    for neg in (dict(n=-1), dict(F=-1), dict(B=-1)):
        assert call(**neg) == -1 and "negative shape" in last_error(lib), neg
    assert call(w=None) == -1 and "null" in last_error(lib)
    assert call(n=0) == 0 and call(B=0) == 0
    for g in (w, sh, pred):
        assert g.untouched()


# ---- xgblinear.train with sequences --------------------------------------------------------

def _bits(models, hist):
    ms = models if isinstance(models, list) else [models]
    return np.stack([np.concatenate([m.weights[:, 0], m.bias]) for m in ms]).tobytes(), np.asarray(hist).tobytes()


@pytest.fixture(scope="module")
def five():
    from expecto_amd.xgblinear import ColMatrix
    X, y, h = make_problem(1003, 33, seed=6, B=5)
    h[:, 0] = 1.0
    return ColMatrix(X), X, y, h


def test_train_sequences_equal_scalar_calls(five):
    from expecto_amd.xgblinear import train
    Xc, X, y, h = five
    kw = dict(eta=HYPER5[:, 0], lambda_=HYPER5[:, 1], alpha=HYPER5[:, 2], lambda_bias=HYPER5[:, 3])
    ev = [(Xc, y[:, ::-1].copy(), h)]
    ms, hist = train(Xc, y, h, num_round=4, evals=ev, **kw)
    assert len(ms) == 5 and hist.shape == (5, 4, 2)
    for m in range(5):
        one, h1 = train(Xc, y[m], h[m], num_round=4, evals=[(Xc, y[m, ::-1].copy(), h[m])],
                        **{k: float(v[m]) for k, v in kw.items()})
        assert _bits(one, h1) == _bits(ms[m], hist[m]), m
    for chunk in (1, 2, 256):
        assert _bits(*train(Xc, y, h, num_round=4, evals=ev, chunk=chunk, **kw)) == _bits(ms, hist), chunk
    # one sequence is enough to make a batch; the floats and the shared y serve every model
    ms2, hist2 = train(Xc, y[0], h[0], num_round=3, eta=0.5, lambda_=[1.0, 10.0, 100.0])
    assert len(ms2) == 3 and hist2.shape == (3, 3, 1)
    for m, lam in enumerate((1.0, 10.0, 100.0)):
        assert _bits(*train(Xc, y[0], h[0], num_round=3, eta=0.5, lambda_=lam)) == _bits(ms2[m], hist2[m])
    with pytest.raises(RuntimeError, match="batch sizes differ"):
        train(Xc, y, h, num_round=1, lambda_=[1.0, 2.0, 3.0])


def test_train_scalars_take_the_old_path_unchanged(five, lib):
    """The recording: the round loop as ``train`` ran it before it learnt about sequences and
    chunks, through expecto_gblinear_train_round, _rmse and _predict_cols directly."""
    import torch
    from expecto_amd import _lib
    from expecto_amd.xgblinear import train
    Xc, X, y, h = five
    B, n, F, R = 5, Xc.n, Xc.F, 4
    yt, ht = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    w = torch.zeros(B, F + 1, device="cuda")
    sh = torch.empty(B, F, dtype=torch.float64, device="cuda")
    pred = torch.empty(B, n, device="cuda")
    hist = torch.zeros(R, B, dtype=torch.float64, device="cuda")

    def rmse(r):
        assert lib.expecto_gblinear_rmse(_lib.dptr(pred), _lib.dptr(yt), n, _lib.dptr(ht), n, n, B, _lib.dptr(hist[r]),
                                         ST()) == 0

    for r in range(R):
        assert lib.expecto_gblinear_train_round(_lib.dptr(Xc.data), Xc.ld, n, F, B, _lib.dptr(yt), n, _lib.dptr(ht), n,
                                                _lib.dptr(w), _lib.dptr(sh), int(r == 0), 0.5, 1.0, 0.25, 0.5, BASE,
                                                _lib.dptr(pred) if r else None, ST()) == 0
        if r:
            rmse(r - 1)
    assert lib.expecto_gblinear_predict_cols(_lib.dptr(Xc.data), Xc.ld, n, F, B, _lib.dptr(w), BASE, _lib.dptr(pred),
                                             ST()) == 0
    rmse(R - 1)
    kw = dict(num_round=R, eta=0.5, lambda_=1.0, alpha=0.25, lambda_bias=0.5)
    ms, got = train(Xc, y, h, **kw)
    assert np.stack([np.concatenate([m.weights[:, 0], m.bias]) for m in ms]).tobytes() == w.cpu().numpy().tobytes()
    assert got[:, :, 0].tobytes() == hist.T.contiguous().cpu().numpy().tobytes()
    for chunk in (1, 2):
        assert _bits(*train(Xc, y, h, chunk=chunk, **kw)) == _bits(ms, got)


# ---- xgblinear.cv --------------------------------------------------------------------------

CV = dict(n=300, F=12, T=2, K=3, R=6, eta=0.5, grid=[(10.0, 2.0), (10.0, 0.0), (0.5, 2.0), (0.5, 0.0)])


@pytest.fixture(scope="module")
def cv_case():
    from expecto_amd.xgblinear import ColMatrix, cv
    X, y, _ = make_problem(CV["n"], CV["F"], seed=77, B=CV["T"])
    fold = np.random.default_rng(78).integers(0, CV["K"], CV["n"])
    Xc = ColMatrix(X)
    res = cv(Xc, y, fold, CV["grid"], num_round=CV["R"], eta=CV["eta"])
    return Xc, X, y, fold, res


def test_cv_equals_single_models(cv_case):
    from expecto_amd.xgblinear import train
    Xc, X, y, fold, res = cv_case
    T, G, K, R = CV["T"], len(CV["grid"]), CV["K"], CV["R"]
    assert res.heldout.shape == res.train.shape == (T, G, K, R) and res.score.shape == res.se.shape == (T, G, R)
    assert res.heldout.dtype == np.float64 and np.isfinite(res.heldout).all() and (res.heldout > 0).all()
    for t in range(T):
        for g, (lam, alpha) in enumerate(CV["grid"]):
            for k in range(K):
                hk, vk = (fold != k).astype(np.float32), (fold == k).astype(np.float32)
                _, hist = train(Xc, y[t], hk, num_round=R, eta=CV["eta"], lambda_=lam, alpha=alpha,
                                evals=[(Xc, y[t], vk)])
                assert_bits(res.train[t, g, k], hist[:, 0].copy(), f"train rmse of model {(t, g, k)}")
                assert_bits(res.heldout[t, g, k], hist[:, 1].copy(), f"held-out rmse of model {(t, g, k)}")
    assert len({res.heldout[0, g].tobytes() for g in range(G)}) == G          # the grid reached the kernel


def test_cv_selection_and_chunks(cv_case):
    from expecto_amd.xgblinear import cv, cv_select
    Xc, X, y, fold, res = cv_case
    score = res.heldout.sum(2) / CV["K"]
    np.testing.assert_allclose(res.score, score, rtol=1e-15)
    for t in range(CV["T"]):
        assert res.score[t, res.best_g[t], res.best_round[t] - 1] == res.score[t].min()
        assert 1 <= res.best_round[t] <= CV["R"]
    for got, want in zip(cv_select(res.heldout, "min"), (res.score, res.se, res.best_g, res.best_round)):
        assert np.array_equal(got, want)
    other = cv(Xc, y, fold, CV["grid"], num_round=CV["R"], eta=CV["eta"], chunk=5, rule="1se")
    assert other.heldout.tobytes() == res.heldout.tobytes() and other.train.tobytes() == res.train.tobytes()
    assert (other.best_g <= res.best_g).all() and other.rule == "1se"
    w3 = np.ones(CV["n"], np.float32) * 3
    weighted = cv(Xc, y[0], fold, CV["grid"][:1], weight=w3, num_round=2, eta=CV["eta"])
    assert weighted.heldout.shape == (1, 1, CV["K"], 2)


def test_cv_refit_equals_plain_train(cv_case):
    from expecto_amd.xgblinear import train
    Xc, X, y, fold, res = cv_case
    models = res.refit(Xc, y)
    assert len(models) == CV["T"]
    for t, m in enumerate(models):
        lam, alpha = res.grid[res.best_g[t]]
        plain, _ = train(Xc, y[t], num_round=int(res.best_round[t]), eta=CV["eta"], lambda_=float(lam),
                         alpha=float(alpha))
        assert _bits(m, 0)[0] == _bits(plain, 0)[0], t


def test_cv_zero_weight_rows_against_removed_rows(cv_case):
    """A fold's model trains on all rows with the held-out ones at weight zero.  Against the numpy
    restatement R32 on the row subset it must lie within noise = max|R32 - R64| of that
    restatement; it need not be bit-equal, the sum tree being indexed by row."""
    from expecto_amd.xgblinear import train
    Xc, X, y, fold, res = cv_case
    lam, alpha = CV["grid"][1]
    keep = fold != 0
    r32, noise, _ = noise_of(X[keep], y[:, keep], None, eta=CV["eta"], lam=lam, alpha=alpha, rounds=CV["R"])
    ms, _ = train(Xc, y, keep.astype(np.float32), num_round=CV["R"], eta=CV["eta"], lambda_=[lam] * CV["T"],
                  alpha=[alpha] * CV["T"])
    got = np.stack([np.concatenate([m.weights[:, 0], m.bias]) for m in ms]).astype(np.float64)
    err = np.abs(got - r32).max(1)
    print(f"zero weights vs R32 on the subset: max err {err}, noise {noise}")
    assert (err <= noise).all(), (err, noise)


# ---- the CLI -------------------------------------------------------------------------------

def test_cli_cv_end_to_end(tmp_path, capsys):
    import pandas as pd
    from expecto_amd import train as cli

    rng = np.random.default_rng(19)
    G = 300
    X = rng.standard_normal((G, 20020)) * rng.uniform(0.01, 3.0, 20020)
    np.save(tmp_path / "X.npy", X)
    chrom = ["chr1", "chr2", "chr8", "chr3", "chrX", "chr4", "chr1", "chrY"]
    anno = pd.DataFrame({"id": [f"G{i}" for i in range(G)], "seqnames": [chrom[i % 8] for i in range(G)],
                         "type": ["rRNA" if i % 10 == 9 else "protein_coding" for i in range(G)]})
    anno.to_csv(tmp_path / "geneanno.csv", index=False)
    exp = pd.DataFrame({"id": anno["id"], "tA": rng.uniform(0.1, 50, G), "tB": rng.uniform(0.1, 50, G)})
    exp.to_csv(tmp_path / "exp.csv", index=False)
    feats = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
    common = ["--expFile", str(tmp_path / "exp.csv"), "--inputFile", str(tmp_path / "X.npy"), "--annoFile",
              str(tmp_path / "geneanno.csv"), "--belugaFeatures", feats, "--no_tf_features", "--eta", "0.5", "--metrics"]
    out = tmp_path / "cv"
    res = cli.run(cli.build_parser(cv=True).parse_args(common + [
        "--targetIndex", "1", "2", "--cv", "3", "--l2-grid", "1", "100", "--l1-grid", "0", "0.5", "--num_round", "5",
        "--output_dir", str(out)]))
    assert [r["name"] for r in res] == ["tA", "tB"]

    folds = pd.read_csv(out / "cv_folds.tsv", sep="\t")
    assert list(folds.columns) == ["chromosome", "fold", "rows"]
    i = np.arange(G)
    tr = np.isin(i % 8, [0, 1, 3, 5, 6]) & (i % 10 != 9)
    rows = {c: int((tr & (np.array([chrom[j % 8] for j in i]) == c)).sum()) for c in ("chr1", "chr2", "chr3", "chr4")}
    assert dict(zip(folds["chromosome"], folds["rows"])) == rows
    # chr1 has twice the rows of the others: it comes first and keeps fold 0 to itself
    assert folds["chromosome"][0] == "chr1" and folds["fold"].tolist()[:3] == [0, 1, 2] and folds["fold"][3] in (1, 2)
    assert folds["rows"].tolist() == sorted(folds["rows"], reverse=True)

    table = pd.read_csv(out / "cv.tsv", sep="\t")
    assert list(table.columns) == ["target", "l2", "l1", "round", "score", "se", "fold0", "fold1", "fold2"]
    assert len(table) == 2 * 4 * 5
    assert table[["l2", "l1"]].drop_duplicates().values.tolist() == [[100.0, 0.5], [100.0, 0.0], [1.0, 0.5], [1.0, 0.0]]
    np.testing.assert_allclose(table["score"], table[["fold0", "fold1", "fold2"]].mean(1), rtol=1e-14)
    best = pd.read_csv(out / "cv_best.tsv", sep="\t")
    assert list(best.columns) == ["target", "l2", "l1", "num_round", "score", "se"] and list(best["target"]) == ["tA", "tB"]
    for _, b in best.iterrows():
        mine = table[table["target"] == b["target"]]
        assert b["score"] == mine["score"].min()
        hit = mine[(mine["l2"] == b["l2"]) & (mine["l1"] == b["l1"]) & (mine["round"] == b["num_round"])]
        assert len(hit) == 1 and hit["score"].iloc[0] == b["score"] and hit["se"].iloc[0] == b["se"]

    cv_metrics = pd.read_csv(out / "metrics" / "metrics.tsv", sep="\t")
    for t, (r, (_, b)) in enumerate(zip(res, best.iterrows())):
        plain_dir = tmp_path / f"plain{t}"
        plain = cli.run(cli.build_parser(cv=True).parse_args(common + [
            "--targetIndex", str(t + 1), "--l2", repr(float(b["l2"])), "--l1", repr(float(b["l1"])), "--num_round",
            str(int(b["num_round"])), "--output_dir", str(plain_dir)]))
        assert len(plain) == 1
        assert os.path.basename(plain[0]["save"]) == os.path.basename(r["save"])
        for ext in ("save", "dump"):
            assert open(plain[0][ext], "rb").read() == open(r[ext], "rb").read(), (t, ext)
        assert plain[0]["history"].tobytes() == np.asarray(r["history"]).tobytes()
        pm = pd.read_csv(plain_dir / "metrics" / "metrics.tsv", sep="\t")
        assert pm.iloc[0].tolist()[2:] == cv_metrics.iloc[t].tolist()[2:]
    text = capsys.readouterr().out
    assert text.count("Cell type: tA") == 2 and text.count("Cell type: tB") == 2

    only = tmp_path / "only"
    assert cli.run(cli.build_parser(cv=True).parse_args(common + ["--targetIndex", "1", "--cv", "4", "--cv-only", "--cv-rule",
                                                           "1se", "--num_round", "2", "--output_dir", str(only)])) == []
    assert sorted(os.listdir(only)) == ["cv.tsv", "cv_best.tsv", "cv_folds.tsv"]
    with pytest.raises(ValueError, match="only 4 chromosomes"):
        cli.run(cli.build_parser(cv=True).parse_args(common + ["--targetIndex", "1", "--cv", "5", "--output_dir", str(only)]))
