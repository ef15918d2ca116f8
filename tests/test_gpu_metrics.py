"""GPU: the metric kernels (expecto_rank2_*, expecto_model_metrics, expecto_bootstrap_coef_stats) through the
C entry points, bit for bit against tests/metrics_ref.py, and the CLIs built on them (train --metrics
--holdout, train_susztak, bootstrap_coefficients) on a synthetic problem.

Every comparison of a kernel's output is equality of bits (``assert_bits``): the ranks and the Spearman sums
are integers, the float64 sums run in the stated order with contraction off, and double division and sqrt are
correctly rounded.  Outputs sit in ``Guarded`` buffers; inputs sit in allocations with NaN margins and NaN
between the rows, so a read past a row poisons a result instead of faulting."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import metrics_ref as ref
from conftest import GOLDEN
from gblinear_ref import make_problem
from guarded import ST, Guarded, assert_bits, dev

pytestmark = pytest.mark.gpu

EINVAL = -1
TILE, LDS_TILE = 256, 2048                 # expecto_amd.metrics.RANK_TILE / RANK_LDS_TILE
N_SET = [1, 2, 63, 64, 65, 255, 256, 257, 1003, 32768]
MARGIN = 4096


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib, metrics
    assert (metrics.RANK_TILE, metrics.RANK_LDS_TILE, metrics.MAX_ROWS) == (TILE, LDS_TILE, 32768)
    return _lib.load()


class Rows:
    """Rows ``a`` ([P, n], float32 or float64) on the device with ``stride`` elements per row (0: one shared
    row), NaN in the gaps and in MARGIN elements before the first and after the last row."""

    def __init__(self, a, stride):
        import torch
        a = np.atleast_2d(a)
        rows, n = a.shape
        assert (stride >= n) if stride else rows == 1
        step = stride if stride else n
        host = np.full(2 * MARGIN + rows * step, np.nan, a.dtype)
        host[MARGIN:MARGIN + rows * step].reshape(rows, step)[:, :n] = a
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + MARGIN * a.dtype.itemsize
        self.stride = stride


_RANKS = {}


def rank_ref(row):
    """ref.rank2_ref, computed once per distinct row of this module."""
    key = (row.dtype.str, row.tobytes())
    if key not in _RANKS:
        _RANKS[key] = ref.rank2_ref(row)
    return _RANKS[key]


def gpu_rank2(lib, a, stride):
    a = np.atleast_2d(a)
    P, n = a.shape
    fn = lib.expecto_rank2_f32 if a.dtype == np.float32 else lib.expecto_rank2_f64
    x = Rows(a, stride)
    out = Guarded((P, n), np.int32)
    assert fn(x.ptr, x.stride, n, P, out.ptr, ST()) == 0, lib.expecto_last_error()
    return out.result()


def untied(n, seed, dtype):
    """n distinct values in random order, exact in float32."""
    return (np.random.default_rng(seed).permutation(n).astype(np.float64) * 0.25 - n / 8.0).astype(dtype)


def rank_rows(n, dtype, P):
    rng = np.random.default_rng([n, P])
    rows = [untied(n, n, dtype), np.round(rng.standard_normal(n) * 3.0), rng.integers(0, 3, n) * 0.5]   # untied, tied, heavily tied
    return np.stack(rows[:P]).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", N_SET)
def test_rank2_sizes(lib, n, dtype):
    P = 1 if n > 2048 else 3
    a = rank_rows(n, dtype, P)
    got = gpu_rank2(lib, a, n + 7)
    assert_bits(got, np.stack([rank_ref(r) for r in a]), f"rank2 n={n}")
    assert got.sum(1).tolist() == [n * (n + 1)] * P


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank2_ties_signed_zero_and_nan(lib, dtype):
    n = LDS_TILE + TILE + 37
    base = untied(n, 5, dtype)
    base[base == 0.0] = 0.125                                        # zeros only where the case puts them
    equal = np.full(n, -2.5, dtype)
    tile = base.copy()
    tile[[TILE - 1, TILE]] = 1e6                                     # a tie across the owners' boundary
    tile[[LDS_TILE - 1, LDS_TILE]] = -1e6                            # and across the LDS tile's
    zeros = base.copy()
    zeros[[3, TILE + 1, LDS_TILE + 5]] = [0.0, -0.0, 0.0]
    nan = base.copy()
    nan[[0, TILE, n - 1]] = np.nan
    a = np.stack([equal, tile, zeros, nan]).astype(dtype)
    got = gpu_rank2(lib, a, n + 1)
    assert_bits(got, np.stack([rank_ref(r) for r in a]), "rank2 special rows")
    assert (got[0] == n + 1).all()
    assert got[1, TILE - 1] == got[1, TILE] == 2 * n - 1 and got[1, LDS_TILE - 1] == got[1, LDS_TILE] == 3
    assert len({int(got[2, i]) for i in (3, TILE + 1, LDS_TILE + 5)}) == 1
    keep = ~np.isnan(a[3])
    assert (got[3, ~keep] == 1).all()
    # the other elements rank as if the NaNs were absent, plus nothing: a NaN is below and equal to no one
    assert_bits(got[3, keep], rank_ref(a[3, keep]), "ranks beside NaN")


def test_rank2_limits(lib):
    out = Guarded((1, 8), np.int32)
    x = Rows(np.zeros((1, 8), np.float32), 8)
    for fn in (lib.expecto_rank2_f32, lib.expecto_rank2_f64):
        assert fn(x.ptr, 8, 32769, 1, out.ptr, ST()) == EINVAL and b"32768" in lib.expecto_last_error()
        assert fn(x.ptr, 8, 8, 65536, out.ptr, ST()) == EINVAL
        assert fn(x.ptr, 8, -1, 1, out.ptr, ST()) == EINVAL
        assert fn(None, 8, 8, 1, out.ptr, ST()) == EINVAL and b"null" in lib.expecto_last_error()
        assert fn(None, 0, 0, 3, None, ST()) == 0 and fn(None, 0, 5, 0, None, ST()) == 0
    assert out.untouched()
    from expecto_amd import metrics
    with pytest.raises(ValueError, match="32768"):
        metrics.rank2(np.zeros(32769, np.float32))
    r = metrics.rank2(np.array([[3.0, 1.0, 3.0], [1.0, 2.0, 3.0]]))
    assert r.dtype.is_floating_point is False and r.cpu().tolist() == [[5, 2, 5], [2, 4, 6]]
    assert metrics.rank2(np.array([0.5, 0.25], np.float32)).cpu().tolist() == [4, 2]


# -- model_metrics ------------------------------------------------------------------------------------------------
def gpu_metrics(lib, pred, y, shared, pred_pad=3, y_pad=5):
    """expecto_model_metrics on guarded buffers, the ranks from expecto_rank2_* on the same device rows."""
    pred = np.atleast_2d(np.asarray(pred, np.float32))
    y = np.atleast_2d(np.asarray(y, np.float64))
    P, n = pred.shape
    assert y.shape == ((1, n) if shared else (P, n))
    pd_, yd = Rows(pred, n + pred_pad), Rows(y, 0 if shared else n + y_pad)
    ra, rb = Guarded((P, n), np.int32), Guarded(y.shape, np.int32)
    assert lib.expecto_rank2_f32(pd_.ptr, pd_.stride, n, P, ra.ptr, ST()) == 0
    assert lib.expecto_rank2_f64(yd.ptr, yd.stride, n, y.shape[0], rb.ptr, ST()) == 0
    out = Guarded((P, 3), np.float64)
    st = lib.expecto_model_metrics(pd_.ptr, pd_.stride, yd.ptr, yd.stride, ra.ptr, rb.ptr, n, P, out.ptr, ST())
    assert st == 0, lib.expecto_last_error()
    ra.result(), rb.result()
    return out.result()


def metrics_want(pred, y, shared):
    """ref.model_metrics_ref with this module's rank cache."""
    pred = np.atleast_2d(np.asarray(pred, np.float32))
    y = np.atleast_2d(np.asarray(y, np.float64))
    out = np.empty((pred.shape[0], 3))
    for m in range(pred.shape[0]):
        ym = y[0] if shared else y[m]
        if np.isnan(pred[m]).any() or np.isnan(ym).any():
            out[m] = np.nan
            continue
        r, r2 = ref.pearson_r2_ref(pred[m], ym)
        out[m] = r, ref.spearman_ref(rank_ref(pred[m]), rank_ref(ym)), r2
    return out


def metric_problem(n, P, shared, seed=0):
    rng = np.random.default_rng([seed, n, P, int(shared)])
    y = rng.standard_normal((1 if shared else P, n)) * 2.0 + 1.0
    pred = (rng.uniform(-1, 1, (P, 1)) * y + rng.standard_normal((P, n)) + 0.5).astype(np.float32)
    if P > 1:
        pred[1] = np.round(pred[1] * 2.0) / 2.0                          # one model with heavy ties
    return pred, y


@pytest.mark.parametrize("P,shared", [(1, True), (1, False), (5, True), (5, False)])
@pytest.mark.parametrize("n", [n for n in N_SET if 2 <= n <= 1003])
def test_model_metrics_sizes(lib, n, P, shared):
    pred, y = metric_problem(n, P, shared)
    assert_bits(gpu_metrics(lib, pred, y, shared), metrics_want(pred, y, shared), f"metrics n={n} P={P}")


@pytest.mark.parametrize("shared", [True, False])
def test_model_metrics_largest_n_untied(lib, shared):
    """n = 32768 without ties: the int64 sums at their largest, against the Python-int restatement."""
    n = 32768
    pred, y = untied(n, 1, np.float32)[None], untied(n, 2, np.float64)[None]
    a, b = rank_ref(pred[0]), rank_ref(y[0])
    assert sorted(a.tolist()) == list(range(2, 2 * n + 1, 2))
    assert n * sum(int(v) ** 2 for v in a) > 2 ** 60                   # the term the header's bound is about
    got = gpu_metrics(lib, pred, y, shared)
    assert_bits(got, metrics_want(pred, y, shared), "metrics n=32768")
    same = gpu_metrics(lib, y.astype(np.float32), y, shared)            # the extreme of n * Sab itself
    assert_bits(same, np.array([[1.0, 1.0, 1.0]]), "pred == y at n=32768")


def test_model_metrics_special_inputs(lib):
    n = 300
    rng = np.random.default_rng(3)
    y = np.round(rng.standard_normal(n) * 8.0) / 8.0                     # exact in float32
    const = np.full(n, 1.25)
    pred = np.stack([np.full(n, 0.75), y, -y, (y + rng.standard_normal(n)), y]).astype(np.float32)
    pred[3, 17] = np.nan
    got = gpu_metrics(lib, pred, y[None], True)
    assert_bits(got, metrics_want(pred, y[None], True), "special pred rows")
    assert np.isnan(got[0, :2]).all() and np.isfinite(got[0, 2])         # constant pred: NaN Spearman and Pearson
    assert got[1].tolist() == [1.0, 1.0, 1.0]                            # pred == y
    assert got[2, 0] == -1.0 and got[2, 1] == -1.0                        # anti-monotone
    assert np.isnan(got[3]).all()                                        # a NaN in pred
    assert got[4].tolist() == [1.0, 1.0, 1.0]
    ys = np.stack([const, const, y, y])
    ys[3, 5] = np.nan
    preds = np.stack([const, const + 0.5, y, y]).astype(np.float32)
    got = gpu_metrics(lib, preds, ys, False)
    assert_bits(got, metrics_want(preds, ys, False), "special y rows")
    assert got[0, 2] == 1.0 and got[1, 2] == 0.0                         # constant y: exact and inexact fit
    assert np.isnan(got[0, :2]).all() and np.isnan(got[1, :2]).all()
    assert got[2].tolist() == [1.0, 1.0, 1.0] and np.isnan(got[3]).all()


def test_model_metrics_limits(lib):
    from expecto_amd import metrics
    out = Guarded((1, 3), np.float64)
    p, y, r = dev(np.zeros(8, np.float32)), dev(np.zeros(8)), dev(np.ones(8, np.int32))
    args = (p.data_ptr(), 8, y.data_ptr(), 0, r.data_ptr(), r.data_ptr())
    for n in (1, 32769, 0, -1):
        assert lib.expecto_model_metrics(*args, n, 1, out.ptr, ST()) == EINVAL, n
    assert b"32768" in lib.expecto_last_error() or b"at least 2" in lib.expecto_last_error()
    assert lib.expecto_model_metrics(*args, 8, -1, out.ptr, ST()) == EINVAL
    assert lib.expecto_model_metrics(None, 8, y.data_ptr(), 0, r.data_ptr(), r.data_ptr(), 8, 1, out.ptr, ST()) == EINVAL
    assert lib.expecto_model_metrics(None, 8, None, 0, None, None, 8, 0, None, ST()) == 0
    assert out.untouched()
    for n in (1, 32769):
        with pytest.raises(ValueError, match="32768"):
            metrics.model_metrics(np.zeros((2, n), np.float32), np.zeros(n))
    with pytest.raises(ValueError):
        metrics.model_metrics(np.zeros((2, 9), np.float32), np.zeros((3, 9)))


def test_model_metrics_wrapper(lib):
    import torch
    from expecto_amd import metrics
    pred, y = metric_problem(1003, 5, True)
    want = metrics_want(pred, y, True)
    assert_bits(metrics.model_metrics(pred, y[0]), want, "host inputs, shared y")
    assert_bits(metrics.model_metrics(torch.from_numpy(pred).cuda(), np.repeat(y, 5, 0)), want, "device pred, [P, n] y")
    assert metrics.model_metrics(np.zeros((0, 9), np.float32), np.zeros(9)).shape == (0, 3)


# -- bootstrap_coef_stats -------------------------------------------------------------------------------------------
def gpu_coef_stats(lib, W, w_main, ld):
    B, F = W.shape
    Wd, wd = Rows(W, ld), Rows(w_main[None], 0)
    outs = [Guarded((F,), np.float64) for _ in range(4)]
    st = lib.expecto_bootstrap_coef_stats(Wd.ptr, ld, B, F, wd.ptr, *[o.ptr for o in outs], ST())
    assert st == 0, lib.expecto_last_error()
    return dict(zip(("mean", "se", "z", "cv"), [o.result() for o in outs]))


@pytest.mark.parametrize("B,F", ref.STATS_CASES)
def test_coef_stats_sizes(lib, B, F):
    W, w_main = ref.stats_case(B, F)
    if F > 4:
        W[:, 1] = 0.03125                      # equal in every model: se = 0, z = +-inf
        W[:, 2] = -0.5
        w_main[2] = 0.0                        # ... and 0 / 0 = NaN for a zero main weight
        W[:, 3] = 0.0                          # mean 0 too: cv = 0 / 0
    want = ref.coef_stats_ref(W, w_main)
    for ld in (F, F + 3):
        got = gpu_coef_stats(lib, W, w_main, ld)
        for k in ("mean", "se", "z", "cv"):
            assert_bits(got[k], want[k], f"coef stats {k} B={B} F={F} ld={ld}")
    if F > 4:
        assert got["se"][1] == 0.0 and np.isinf(got["z"][1]) and np.isnan(got["z"][2]) and np.isnan(got["cv"][3])
    with open(os.path.join(GOLDEN, "metrics", "values.json")) as f:
        g = next(s for s in json.load(f)["stats"] if (s["B"], s["F"]) == (B, F))
    if F <= 4:                                  # untouched columns: numpy's own figures, bit for bit
        assert got["mean"].tolist() == g["mean"] and got["se"].tolist() == g["std_ddof1"]
    else:
        assert got["mean"][4:].tolist() == g["mean"][4:] and got["se"][4:].tolist() == g["std_ddof1"][4:]


def test_coef_stats_limits(lib):
    from expecto_amd import metrics
    W, w = dev(np.ones((2, 4))), dev(np.ones(4))
    outs = [Guarded((4,), np.float64) for _ in range(4)]
    ptrs = [o.ptr for o in outs]
    for B in (1, 4097, 0):
        assert lib.expecto_bootstrap_coef_stats(W.data_ptr(), 4, B, 4, w.data_ptr(), *ptrs, ST()) == EINVAL, B
        assert b"4096" in lib.expecto_last_error()
    assert lib.expecto_bootstrap_coef_stats(W.data_ptr(), 3, 2, 4, w.data_ptr(), *ptrs, ST()) == EINVAL
    assert lib.expecto_bootstrap_coef_stats(None, 4, 2, 4, w.data_ptr(), *ptrs, ST()) == EINVAL
    assert lib.expecto_bootstrap_coef_stats(None, 0, 2, 0, None, None, None, None, None, ST()) == 0
    assert all(o.untouched() for o in outs)
    for B in (1, 4097):
        with pytest.raises(ValueError, match="4096"):
            metrics.bootstrap_coef_stats(np.ones((B, 4)), np.ones(4))
    Wh, wh = ref.stats_case(3, 257)
    got, want = metrics.bootstrap_coef_stats(Wh, wh), ref.coef_stats_ref(Wh, wh)
    for k in want:
        assert_bits(got[k], want[k], f"wrapper {k}")


# -- the CLIs -------------------------------------------------------------------------------------------------------
G, F_MARKS = 320, 2
CHROMS = ["chr1", "chr7", "chr8", "chrX", "chr1", "chr1", "chr8", "chr7"]
TARGETS = ["tA", "tB", "tC"]

# stdout of `train --targetIndex all --no_tf_features --num_round 3` on make_cli_problem's files, as the commit
# before --metrics / --holdout printed it (captured once on an MI355X)
PARENT_STDOUT = """\
not including TF features
Number of features included in model: 2
Training data shape: (320, 20)
Cell type: tA
[0]\teval-rmse:2.189521\ttrain-rmse:2.096802
[1]\teval-rmse:2.172871\ttrain-rmse:2.079152
[2]\teval-rmse:2.156382\ttrain-rmse:2.061690
SignificanceResult(statistic=np.float64(0.9419596812001877), pvalue=np.float64(1.0153399518056724e-38))
Cell type: tB
[0]\teval-rmse:2.483205\ttrain-rmse:2.179252
[1]\teval-rmse:2.464797\ttrain-rmse:2.160637
[2]\teval-rmse:2.446593\ttrain-rmse:2.142262
SignificanceResult(statistic=np.float64(0.9149085794655416), pvalue=np.float64(1.8255405478118966e-32))
Cell type: tC
[0]\teval-rmse:1.240829\ttrain-rmse:1.163592
[1]\teval-rmse:1.230914\ttrain-rmse:1.153926
[2]\teval-rmse:1.221109\ttrain-rmse:1.144369
SignificanceResult(statistic=np.float64(0.8237458977965307), pvalue=np.float64(6.504453236550874e-21))
"""


def make_cli_problem(root):
    """A few hundred genes over chr1, chr7, chr8 and chrX, 3 expression columns, 2 marks kept of 2002 (F = 20):
    files under ``root``; returns the argument list every CLI here shares."""
    import pandas as pd
    X, y, _ = make_problem(G, 10 * F_MARKS, seed=21, B=3)
    keep = [7, 1500]
    full = np.zeros((G, 10, 2002), np.float32)
    full[:, :, keep] = X.reshape(G, 10, F_MARKS)
    np.save(os.path.join(root, "X.npy"), full.reshape(G, -1))
    anno = pd.DataFrame({"id": [f"G{i}" for i in range(G)], "seqnames": [CHROMS[i % 8] for i in range(G)],
                         "type": ["rRNA" if i % 16 == 5 else "protein_coding" for i in range(G)]})
    anno.to_csv(os.path.join(root, "geneanno.csv"), index=False)
    exp = pd.DataFrame({"id": anno["id"], **{t: np.exp(y[k].astype(np.float64) * 0.5) for k, t in enumerate(TARGETS)}})
    exp.to_csv(os.path.join(root, "exp.csv"), index=False)
    marks = pd.DataFrame({"Cell type": [f"c{i % 9}" for i in range(2002)],
                          "Assay": [f"a{i}" for i in range(2002)],
                          "Assay type": ["DNase" if i in keep else "TF" for i in range(2002)]})
    marks.to_csv(os.path.join(root, "features.tsv"), sep="\t")
    return ["--expFile", os.path.join(root, "exp.csv"), "--inputFile", os.path.join(root, "X.npy"), "--annoFile",
            os.path.join(root, "geneanno.csv"), "--belugaFeatures", os.path.join(root, "features.tsv"),
            "--num_round", "3", "--no_tf_features"]


def _captured(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fn(*a, **kw)
    return res, buf.getvalue()


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from expecto_amd import train, train_susztak
    root = str(tmp_path_factory.mktemp("metrics_cli"))
    common = make_cli_problem(root)
    runs = {"root": root, "common": common}
    p = train.build_parser()
    runs["plain"] = _captured(train.run, p.parse_args(common + ["--targetIndex", "all", "--output_dir", root + "/plain"]))
    runs["metrics"] = _captured(train.run, p.parse_args(
        common + ["--targetIndex", "all", "--holdout", "chr7", "--metrics", "--output_dir", root + "/metrics"]))
    runs["susztak"] = _captured(train_susztak.run, train_susztak.build_parser().parse_args(
        common + ["--output_dir", root + "/susztak"]))
    runs["boot"] = _captured(train.run, p.parse_args(
        common + ["--targetIndex", "1", "--n_bootstrap", "4", "--seed", "3", "--output_dir", root + "/boot/run1"]))
    return runs


def _rows_of(root, ti, holdout):
    """(X [G, 20] float32, ylog float64, train mask, test mask) from the files, by the chromosome names."""
    import pandas as pd
    anno, exp = pd.read_csv(root + "/geneanno.csv"), pd.read_csv(root + "/exp.csv")
    X = np.load(root + "/X.npy").reshape(G, 10, 2002)[:, :, [7, 1500]].reshape(G, -1)
    ok = (anno["type"] != "rRNA").to_numpy()
    chrom = anno["seqnames"].to_numpy()
    tr = ok & ~np.isin(chrom, ["chrX", "chrY", "chr8"] + list(holdout))
    return X, np.log(exp.iloc[:, ti].to_numpy() + 0.0001), tr, ok & (chrom == "chr8")


def test_cli_metrics_files(cli):
    from expecto_amd import h5
    from expecto_amd.metrics import model_metrics
    from expecto_amd.train import METRIC_NAMES
    from expecto_amd.xgblinear import ColMatrix, predict_cols
    root = cli["root"]
    res, _ = cli["metrics"]
    assert [(r["name"], r["boot"]) for r in res] == [(t, None) for t in TARGETS]
    back = h5.read(root + "/metrics/metrics/metrics.h5")
    assert sorted(back) == sorted(METRIC_NAMES) and len(back) == 6
    with open(os.path.join(GOLDEN, "metrics", "values.json")) as f:
        lib_p, lib_r = ref.library_errors(json.load(f)["pairs"])
    tsv = [l.split("\t") for l in open(root + "/metrics/metrics/metrics.tsv").read().splitlines()]
    assert tsv[0] == ["name", "boot"] + list(METRIC_NAMES) and [l[0] for l in tsv[1:]] == TARGETS
    for k in METRIC_NAMES:
        assert back[k].dtype == np.float64 and back[k].shape == (3,)
    for m, r in enumerate(res):
        X, ylog, tr, te = _rows_of(root, 1 + m, ["chr7"])
        assert tr.sum() == 100 and te.sum() == 80
        for rows, tag in ((tr, "trains"), (te, "valids")):
            pred = predict_cols(ColMatrix(X[rows]), r["model"])
            got = np.array([back[f"{s}_{tag}"][m] for s in ("pearsonr", "spearmanr", "r2")])
            assert_bits(got, model_metrics(pred[None], ylog[rows])[0], f"{r['name']} {tag} vs model_metrics")
            assert_bits(got, ref.model_metrics_ref(pred.cpu().numpy(), ylog[rows])[0], f"{r['name']} {tag} vs ref")
            assert [r["metrics"][f"{s}_{tag}"] for s in ("pearsonr", "spearmanr", "r2")] == got.tolist()
            assert [float(v) for v in tsv[1 + m][2 + (tag == "valids")::2]] == got.tolist()
            try:
                from scipy.stats import pearsonr, spearmanr
                from sklearn.metrics import r2_score
            except ImportError:
                continue
            p = pred.cpu().numpy()
            d = [abs(got[0] - pearsonr(ylog[rows], p)[0]), abs(got[1] - spearmanr(ylog[rows], p)[0]),
                 abs(got[2] - r2_score(y_true=ylog[rows], y_pred=p))]
            print(f"{r['name']} {tag}: |pearson - scipy| {d[0]:.3g}, |spearman - scipy| {d[1]:.3g}, |r2 - sklearn| {d[2]:.3g}")
            assert d[0] <= 4 * lib_p and d[2] <= 4 * lib_r and d[1] <= 4 * 2.0 ** -53


def test_cli_holdout_changes_the_training_rows(cli):
    from expecto_amd.train import select_rows
    import pandas as pd
    root = cli["root"]
    anno, exp = pd.read_csv(root + "/geneanno.csv"), pd.read_csv(root + "/exp.csv")
    tr, te = select_rows(anno, exp.iloc[:, 1], "all", 0.0001, ["chr7"])
    _, _, want_tr, want_te = _rows_of(root, 1, ["chr7"])
    assert tr.tolist() == want_tr.tolist() and te.tolist() == want_te.tolist()
    assert not (anno["seqnames"].to_numpy()[tr] == "chr7").any()
    plain, held = cli["plain"][0], cli["metrics"][0]
    assert all(a["model"].weights.tobytes() != b["model"].weights.tobytes() for a, b in zip(plain, held))


def test_cli_without_flags_is_unchanged(cli):
    root = cli["root"]
    res, text = cli["plain"]
    assert not os.path.exists(root + "/plain/metrics") and all("metrics" not in r for r in res)
    assert sorted(os.listdir(root + "/plain")) == sorted(
        f"expecto_all.pseudocount0.0001.lambda100.round3.basescore2.{t}.{e}" for t in TARGETS for e in ("save", "dump"))
    try:
        import scipy  # noqa: F401
        drop = ()
    except ImportError:                            # the Spearman line is scipy's repr; without scipy it is another
        drop = ("SignificanceResult", "SpearmanrResult")
    lines = lambda s: [l for l in s.splitlines() if not l.startswith(drop)] if drop else s.splitlines()
    assert lines(text) == lines(PARENT_STDOUT)
    assert cli["metrics"][1].count("\n") == text.count("\n")            # --metrics prints nothing more


def test_cli_train_susztak_equals_train(cli):
    from expecto_amd import h5
    root = cli["root"]
    res, text = cli["susztak"]
    want, want_text = cli["metrics"]
    assert text == want_text
    for a, b in zip(res, want):
        assert a["name"] == b["name"] and a["metrics"] == b["metrics"]
        assert os.path.dirname(a["save"]) == root + "/susztak/models"
        assert os.path.basename(a["save"]) == f"expecto_all.pseudocount0.0001.lambda100.round3.basescore2.{a['name']}.save"
        assert open(a["save"], "rb").read() == open(b["save"], "rb").read()
        assert open(a["dump"]).read() == open(b["dump"]).read()
    a, b = h5.read(root + "/susztak/metrics/metrics.h5"), h5.read(root + "/metrics/metrics/metrics.h5")
    assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert open(root + "/susztak/metrics/metrics.tsv").read() == open(root + "/metrics/metrics/metrics.tsv").read()


def test_cli_bootstrap_coefficients(cli, capsys):
    import pandas as pd
    from expecto_amd import bootstrap_coefficients as bc
    from expecto_amd.xgblinear import GBLinear
    root = cli["root"]
    boots = cli["boot"][0]
    assert [r["boot"] for r in boots] == [0, 1, 2, 3]
    main_model = cli["plain"][0][0]["save"]
    F = 10 * F_MARKS
    clusters = pd.DataFrame({"mark": [f"m{i}" for i in range(F)], "cluster": np.arange(F) % 4},
                            index=[f"f{i}" for i in range(F)])
    clusters.to_csv(root + "/clusters.tsv", sep="\t")
    args = bc.build_parser().parse_args(["--bootstrap_model_dir", root + "/boot", "--main_model", main_model,
                                         "--feature_clusters_df", root + "/clusters.tsv", "-o", root + "/zs",
                                         "--coorFile", "unused", "--maxshift", "800", "--splitFlag"])
    assert args.max_models == 800
    out = bc.run(args)
    assert out["files"] == [r["save"] for r in boots]

    W = np.vstack([GBLinear.load(r["save"]).dump_weights() for r in boots])
    w_main = GBLinear.load(main_model).dump_weights()
    want = ref.coef_stats_ref(W, w_main)
    for k in want:
        assert_bits(out["stats"][k], want[k], f"bootstrap_coefficients {k}")
    df = pd.read_csv(root + "/clusters.tsv", sep="\t", index_col=0)
    df["z_score"] = want["z"]
    df = df.iloc[ref.zscore_order(want["z"])].reset_index(drop=True)
    df.to_csv(root + "/want.csv", sep="\t")
    assert open(root + "/zs/input_features_sorted_by_zscore.csv").read() == open(root + "/want.csv").read()
    stats = pd.read_csv(root + "/zs/coefficient_stats.tsv", sep="\t", index_col=0, float_precision="round_trip")
    assert list(stats.columns) == ["mean", "se", "z_score", "cv"] and stats.shape == (F, 4)
    assert_bits(stats["se"].to_numpy(), want["se"], "coefficient_stats.tsv se")
    printed = capsys.readouterr().out
    top = np.argsort(want["cv"])[-10:][::-1]
    assert "Largest coefficients of variation: " + " ".join(str(int(i)) for i in top) in printed

    clusters.iloc[:-1].to_csv(root + "/short.tsv", sep="\t")
    args.feature_clusters_df = root + "/short.tsv"
    with pytest.raises(ValueError, match="num_feature = 20"):
        bc.run(args)
    two = bc.build_parser().parse_args(["--bootstrap_model_dir", root + "/boot", "--main_model", main_model,
                                        "--feature_clusters_df", root + "/clusters.tsv", "-o", root + "/zs2",
                                        "--max_models", "2"])
    assert len(bc.run(two)["files"]) == 2
