"""CPU: the numpy restatements of tests/metrics_ref.py (what test_gpu_metrics.py holds the kernels to, bit
for bit) against scipy, sklearn and numpy as recorded in tests/golden/metrics/values.json, and the host-side
rules of the new CLIs.

Bars.  Ranks: equality.  Spearman: 4 * 2^-53 absolute, the integer formula's three roundings (two int64 ->
float64 conversions under the root count as one product, the root, the division) plus scipy's own.  Pearson
and R2: four times the largest difference between scipy / sklearn and an extended-precision (np.longdouble)
evaluation of the same formulas over the same cases, i.e. the reference library's own rounding; measured
with scipy 1.15.3: scipy's Pearson is within 1.39e-16 and sklearn's R2 within 1.22e-16 of the extended value,
the restatement within 3.33e-16 and 2.22e-16 of them, and its Spearman within 1.11e-16 of scipy's (all
printed by the tests).  Coefficient statistics: equality of
bits with np.mean / np.std(axis=0, ddof=1), which reduce axis 0 row by row."""
import hashlib
import json
import os

import numpy as np
import pandas as pd
import pytest

import metrics_ref as ref
from conftest import GOLDEN

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "metrics", "values.json")) as f:
        g = json.load(f)
    assert [(p["n"], p["ties"]) for p in g["pairs"]] == ref.PAIR_CASES
    assert [(s["B"], s["F"]) for s in g["stats"]] == ref.STATS_CASES
    return g


@pytest.fixture(scope="module")
def pairs(golden):
    """Per case: inputs, the restatement's ranks and figures, the golden entry, the extended-precision values."""
    out = []
    for g in golden["pairs"]:
        pred, y = ref.pair_case(g["n"], g["ties"])
        ra, rb = ref.rank2_ref(pred), ref.rank2_ref(y)
        r, r2 = ref.pearson_r2_ref(pred, y)
        out.append(dict(g=g, pred=pred, y=y, ra=ra, rb=rb, pearson=r, r2=r2, spearman=ref.spearman_ref(ra, rb),
                        ))
    return out


def _same_ranks(got, want):
    if isinstance(want, dict):
        return hashlib.sha256(got.astype("<i4").tobytes()).hexdigest() == want["sha256"]
    return got.tolist() == want


def test_doubled_ranks_equal_twice_rankdata(pairs):
    for c in pairs:
        assert c["ra"].dtype == np.int32
        assert _same_ranks(c["ra"], c["g"]["rank2_pred"]), (c["g"]["n"], c["g"]["ties"], "pred")
        assert _same_ranks(c["rb"], c["g"]["rank2_y"]), (c["g"]["n"], c["g"]["ties"], "y")
    tied = [c for c in pairs if c["g"]["ties"]]
    assert all(len(set(c["ra"].tolist())) < c["g"]["n"] // 2 for c in tied if c["g"]["n"] > 100)   # heavy ties


def test_spearman_integer_formula_against_scipy(pairs):
    diff = [abs(float(c["spearman"]) - c["g"]["spearmanr"]) for c in pairs]
    print("spearman: max |restatement - scipy| = %.3g (bar %.3g)" % (max(diff), 4 * EPS))
    assert max(diff) <= 4 * EPS


def test_pearson_and_r2_against_scipy_and_sklearn(golden, pairs):
    lib_p, lib_r = ref.library_errors(golden["pairs"])
    got_p = max(abs(float(c["pearson"]) - c["g"]["pearsonr"]) for c in pairs)
    got_r = max(abs(float(c["r2"]) - c["g"]["r2_score"]) for c in pairs)
    print("pearson: scipy vs extended %.3g, restatement vs scipy %.3g" % (lib_p, got_p))
    print("r2: sklearn vs extended %.3g, restatement vs sklearn %.3g" % (lib_r, got_r))
    assert lib_p > 0 and lib_r > 0
    assert got_p <= 4 * lib_p
    assert got_r <= 4 * lib_r


def test_model_metrics_ref_rows(pairs):
    c = pairs[2]
    both = ref.model_metrics_ref(np.stack([c["pred"], -c["pred"]]), c["y"])
    assert both[0].tolist() == [float(c["pearson"]), float(c["spearman"]), float(c["r2"])]
    assert both[1, 0] == -both[0, 0] and both[1, 1] == -both[0, 1]
    bad = c["pred"].copy()
    bad[5] = np.nan
    assert np.isnan(ref.model_metrics_ref(bad, c["y"])).all()


def test_coefficient_statistics_bit_equal_numpy(golden):
    for g in golden["stats"]:
        W, w_main = ref.stats_case(g["B"], g["F"])
        s = ref.coef_stats_ref(W, w_main)
        assert s["mean"].tolist() == g["mean"], (g["B"], g["F"])
        assert s["se"].tolist() == g["std_ddof1"], (g["B"], g["F"])
        assert np.array_equal(s["z"], w_main / np.asarray(g["std_ddof1"]))
        assert np.array_equal(s["cv"], np.asarray(g["std_ddof1"]) / np.abs(np.asarray(g["mean"])))


def test_r2_force_finite_and_constant_inputs():
    y = np.full(40, 1.25)
    assert ref.pearson_r2_ref(y.astype(np.float32), y)[1] == 1.0                 # constant y, exact fit
    r, r2 = ref.pearson_r2_ref((y + 0.5).astype(np.float32), y)                  # constant y, inexact fit
    assert r2 == 0.0 and np.isnan(r)
    x = np.arange(40, dtype=np.float32)
    r, r2 = ref.pearson_r2_ref(np.full(40, 3.0, np.float32), x.astype(np.float64))   # constant pred
    assert np.isnan(r) and np.isfinite(r2)
    assert np.isnan(ref.spearman_ref(ref.rank2_ref(np.full(40, 3.0)), ref.rank2_ref(x)))
    assert ref.model_metrics_ref(x, x.astype(np.float64)).tolist() == [[1.0, 1.0, 1.0]]
    assert ref.spearman_ref(ref.rank2_ref(-x), ref.rank2_ref(x)) == -1.0


def test_rank2_ref_special_values():
    assert ref.rank2_ref(np.array([0.0, -0.0, 1.0])).tolist() == [3, 3, 6]           # -0.0 ties with 0.0
    assert ref.rank2_ref(np.array([2.0, np.nan, 1.0, 2.0])).tolist() == [5, 1, 2, 5]  # NaN compares false
    assert ref.rank2_ref(np.full(5, 7.0, np.float32)).tolist() == [6] * 5


def test_natural_sort_order():
    from expecto_amd.bootstrap_coefficients import natsorted
    names = ["d/run10/m.boot10.save", "d/run2/m.boot1.save", "d/run2/m.boot10.save", "d/run2/m.boot2.save",
             "d/run1/m.save", "d/run1/a12b3.save", "d/run1/a2b30.save", "d/run1/a2b4.save"]
    assert natsorted(names) == ["d/run1/a2b4.save", "d/run1/a2b30.save", "d/run1/a12b3.save", "d/run1/m.save",
                                "d/run2/m.boot1.save", "d/run2/m.boot2.save", "d/run2/m.boot10.save",
                                "d/run10/m.boot10.save"]


def test_stable_zscore_sort_with_ties_and_nan():
    from expecto_amd.bootstrap_coefficients import sort_by_zscore
    z = np.array([1.0, -3.0, np.nan, 3.0, -1.0, np.inf, 0.0, np.nan, -np.inf])
    assert ref.zscore_order(z).tolist() == [5, 8, 1, 3, 0, 4, 6, 2, 7]
    df = pd.DataFrame({"mark": [f"m{i}" for i in range(9)], "cluster": np.arange(9) % 3},
                      index=[f"row{i}" for i in range(9)])
    out = sort_by_zscore(df, z)
    assert list(out.columns) == ["mark", "cluster", "z_score"]
    assert out.index.tolist() == list(range(9))
    assert out["mark"].tolist() == [f"m{i}" for i in ref.zscore_order(z)]
    assert np.array_equal(out["z_score"].to_numpy(), z[ref.zscore_order(z)], equal_nan=True)
    assert "temp" not in df.columns and "z_score" not in df.columns            # the input frame is left alone


def _anno():
    chrom = ["chr1", "chr7", "chr8", "chrX", "chr2", "chrY", "chr7", "chr8"]
    return pd.DataFrame({"id": [f"G{i}" for i in range(16)], "seqnames": chrom * 2,
                         "type": ["rRNA" if i == 4 else "protein_coding" for i in range(16)]})


def test_holdout_row_masks():
    from expecto_amd.train import select_rows
    anno = _anno()
    expr = pd.Series(np.r_[np.full(15, 2.0), -1.0])           # the last gene's log is not finite
    tr0, te0 = select_rows(anno, expr, "all", 0.0001)
    tr0b, te0b = select_rows(anno, expr, "all", 0.0001, ())
    tr7, te7 = select_rows(anno, expr, "all", 0.0001, ["chr7"])
    tr72, _ = select_rows(anno, expr, "all", 0.0001, ["chr7", "chr2"])
    chrom = anno["seqnames"].to_numpy()
    assert tr0.tolist() == tr0b.tolist() and te0.tolist() == te0b.tolist()
    assert np.nonzero(tr0)[0].tolist() == [0, 1, 6, 8, 9, 12, 14]
    assert np.nonzero(tr7)[0].tolist() == [0, 8, 12]
    assert np.nonzero(tr72)[0].tolist() == [0, 8]
    assert not (chrom[tr7] == "chr7").any() and (chrom[tr0] == "chr7").any()
    assert te7.tolist() == te0.tolist() and np.nonzero(te7)[0].tolist() == [2, 7, 10]


def test_train_arguments_keep_their_defaults():
    from expecto_amd import train, train_susztak
    ns = vars(train.build_parser().parse_args(["--targetIndex", "1"]))
    before = dict(targetIndex=["1"], expFile=None, belugaFeatures=None, inputFile="./resources/Xreducedall.2002.npy",
                  annoFile="./resources/geneanno.csv", evalFile="", filterStr="all", pseudocount=0.0001, num_round=100,
                  l2=100, l1=0, eta=0.01, base_score=2, threads=16, no_tf_features=False, no_dnase_features=False,
                  no_histone_features=False, intersect_with_lambert=False, no_pol2=False,
                  output_dir="temp_expecto_model", n_bootstrap=0, seed=0)
    assert list(ns)[:len(before)] == list(before)             # the same attributes in the same order
    assert {k: ns[k] for k in before} == before
    assert {k: ns[k] for k in ns if k not in before} == {"holdout": [], "metrics": False}
    on = train.build_parser().parse_args(["--targetIndex", "all", "--holdout", "chr7", "chr9", "--metrics"])
    assert on.holdout == ["chr7", "chr9"] and on.metrics is True
    sus = vars(train_susztak.build_parser().parse_args([]))
    assert sus == {k: v for k, v in before.items() if k not in ("targetIndex", "n_bootstrap", "seed")}
