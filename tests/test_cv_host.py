"""CPU: the host side of cross-validated gblinear training -- the chromosome folds and the penalty
grid of the train CLI, both selection rules of xgblinear.cv_select on hand-made held-out rmse, and
the argument checks, all of which refuse before anything touches a device."""
import numpy as np
import pytest

from expecto_amd import train as cli
from expecto_amd import xgblinear


# ---- folds ---------------------------------------------------------------------------------

# rows per chromosome; chrB / chrC and chrE / chrF tie in size
CHROMS = {"chrA": 9, "chrB": 6, "chrC": 6, "chrD": 4, "chrE": 2, "chrF": 2, "chrG": 1}


def _seqnames(seed):
    names = np.repeat(list(CHROMS), list(CHROMS.values()))
    return names[np.random.default_rng(seed).permutation(names.size)]


def test_folds_balance_and_ties():
    """By hand, K = 3, fold sizes in brackets: A(9) -> 0 [9, 0, 0]; B(6) -> 1 [9, 6, 0]; C(6) -> 2 [9, 6, 6];
    D(4): folds 1 and 2 tie at 6 -> 1 [9, 10, 6]; E(2) -> 2 [9, 10, 8]; F(2) -> 2 [9, 10, 10]; G(1) -> 0."""
    seq = _seqnames(0)
    fold, table = cli.chromosome_folds(seq, 3)
    assert table == [("chrA", 0, 9), ("chrB", 1, 6), ("chrC", 2, 6), ("chrD", 1, 4), ("chrE", 2, 2), ("chrF", 2, 2),
                     ("chrG", 0, 1)]
    assert fold.dtype == np.int64 and fold.shape == seq.shape
    of = dict((c, k) for c, k, _ in table)
    assert all(fold[i] == of[s] for i, s in enumerate(seq))
    assert np.bincount(fold).tolist() == [10, 10, 10]


def test_folds_do_not_depend_on_row_order():
    a, b = _seqnames(1), _seqnames(2)
    fa, ta = cli.chromosome_folds(a, 4)
    fb, tb = cli.chromosome_folds(b, 4)
    assert ta == tb == cli.chromosome_folds(a, 4)[1]
    assert dict(zip(a, fa)) == dict(zip(b, fb))
    assert set(fa) == {0, 1, 2, 3}


def test_folds_equal_sizes_go_by_name_and_lowest_fold():
    fold, table = cli.chromosome_folds(["chr2", "chr10", "chr1", "chr3"], 2)
    assert table == [("chr1", 0, 1), ("chr10", 1, 1), ("chr2", 0, 1), ("chr3", 1, 1)]
    assert fold.tolist() == [0, 1, 0, 1]


def test_folds_too_few_chromosomes():
    with pytest.raises(ValueError, match="only 7 chromosomes"):
        cli.chromosome_folds(_seqnames(0), 8)
    assert len(cli.chromosome_folds(_seqnames(0), 7)[1]) == 7
    with pytest.raises(ValueError, match="at least 2"):
        cli.chromosome_folds(_seqnames(0), 1)


# ---- grid ----------------------------------------------------------------------------------

def test_grid_runs_from_most_to_least_regularised():
    assert cli.penalty_grid([1, 100, 10], [0, 0.5]) == [(100.0, 0.5), (100.0, 0.0), (10.0, 0.5), (10.0, 0.0),
                                                         (1.0, 0.5), (1.0, 0.0)]
    assert cli.penalty_grid([100.0], [0.0]) == [(100.0, 0.0)]
    args = cli.build_parser(cv=True).parse_args(["--targetIndex", "1", "--cv", "3", "--l2-grid", "1", "100", "--l1-grid",
                                          "0", "0.5"])
    assert args.cv == 3 and args.l2_grid == [1.0, 100.0] and args.l1_grid == [0.0, 0.5]
    assert args.cv_rule == "min" and not args.cv_only
    off = cli.build_parser(cv=True).parse_args(["--targetIndex", "1"])
    assert off.cv == 0 and off.l2_grid is None and off.l1_grid is None


# ---- selection -----------------------------------------------------------------------------

def _heldout(score, spread):
    """[G, R] means and per-entry spreads -> [1, G, 3, R] with folds mean - s, mean, mean + s
    (exact in binary for the values used here)."""
    score, spread = np.asarray(score, float), np.asarray(spread, float)
    return np.stack([score - spread, score, score + spread], 1)[None]


def test_select_score_and_se():
    ho = np.array([[[[1.0, 4.0], [2.0, 4.0], [6.0, 4.0]]]])             # T = G = 1, K = 3, R = 2
    score, se, g, r = xgblinear.cv_select(ho, "min")
    assert score.shape == se.shape == (1, 1, 2)
    assert score[0, 0].tolist() == [3.0, 4.0]
    assert se[0, 0, 0] == np.sqrt(((1 - 3) ** 2 + (2 - 3) ** 2 + (6 - 3) ** 2) / 2) / np.sqrt(3) and se[0, 0, 1] == 0
    assert g.tolist() == [0] and r.tolist() == [1]


def test_select_min_ties_go_to_the_earlier_grid_entry_then_round():
    score = [[3.0, 2.0, 2.0, 2.5],         # least 2.0 at rounds 2 and 3 (1-based)
             [2.0, 2.0, 4.0, 4.0],         # the same least at rounds 1 and 2
             [5.0, 1.5, 1.5, 9.0]]
    ho = _heldout(score, np.full((3, 4), 0.5))
    _, _, g, r = xgblinear.cv_select(ho[:, :2], "min")
    assert (g.tolist(), r.tolist()) == ([0], [2])                        # tie across entries 0 and 1: entry 0, round 2
    _, _, g, r = xgblinear.cv_select(ho[:, [1, 0]], "min")
    assert (g.tolist(), r.tolist()) == ([0], [1])                        # swapped: still the first entry, its round 1
    _, _, g, r = xgblinear.cv_select(ho, "min")
    assert (g.tolist(), r.tolist()) == ([2], [2])


def test_select_1se_prefers_the_earlier_entry_within_one_se():
    score = [[4.0, 3.0, 3.5],              # most regularised: best 3.0 at round 2
             [4.0, 2.75, 2.5],             # best 2.5 at round 3
             [2.0, 3.0, 3.0]]              # least of all: 2.0 at round 1
    spread = np.zeros((3, 3))
    spread[2, 0] = 1.0                     # folds 1, 2, 3: sd 1, se = 1 / sqrt(3) = 0.577
    ho = _heldout(score, spread)
    sc, se, g, r = xgblinear.cv_select(ho, "min")
    assert (g.tolist(), r.tolist()) == ([2], [1]) and se[0, 2, 0] == 1 / np.sqrt(3)
    _, _, g, r = xgblinear.cv_select(ho, "1se")
    assert (g.tolist(), r.tolist()) == ([1], [3])                        # 2.5 <= 2.577 < 3.0: entry 1, its own round
    spread[2, 0] = 2.0                     # se 1.155: entry 0's 3.0 is inside as well
    _, _, g, r = xgblinear.cv_select(_heldout(score, spread), "1se")
    assert (g.tolist(), r.tolist()) == ([0], [2])
    spread[2, 0] = 0.0                     # se 0: only an exact tie is inside
    _, _, g, r = xgblinear.cv_select(_heldout(score, spread), "1se")
    assert (g.tolist(), r.tolist()) == ([2], [1])


def test_select_per_target_and_nan_never_wins():
    a = _heldout([[3.0, 2.0], [1.0, 5.0]], np.zeros((2, 2)))
    b = _heldout([[np.nan, 2.0], [np.nan, np.nan]], np.zeros((2, 2)))
    _, _, g, r = xgblinear.cv_select(np.concatenate([a, b]), "min")
    assert (g.tolist(), r.tolist()) == ([1, 0], [1, 2])
    with pytest.raises(RuntimeError, match="no finite"):
        xgblinear.cv_select(_heldout([[np.nan]], [[0.0]]), "min")
    with pytest.raises(ValueError, match="rule"):
        xgblinear.cv_select(a, "best")


# ---- argument checks -----------------------------------------------------------------------

X4 = np.zeros((4, 2), np.float32)
Y4 = np.zeros(4, np.float32)


@pytest.mark.parametrize("kw", [dict(lambda_=-1.0), dict(alpha=float("nan")), dict(lambda_bias=-0.5),
                                dict(eta=float("inf")), dict(lambda_=[1.0, -2.0]), dict(alpha=[0.0, float("nan")]),
                                dict(eta=[0.1, float("nan")]), dict(lambda_=[[1.0, 2.0]])])
def test_train_refuses_bad_hyper_parameters_on_the_host(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        xgblinear.train(X4, Y4, **kw)


def test_hyper_table():
    hp, B = xgblinear._hyper(0.5, 1.0, 0.0, 0.0)
    assert hp == (0.5, 1.0, 0.0, 0.0) and B is None
    hp, B = xgblinear._hyper(0.5, [1.0, 2.0, 3.0], 0.0, np.array([0.0, 0.25, 0.5]))
    assert B == 3 and hp.dtype == np.float64 and hp.flags.c_contiguous
    assert hp.tolist() == [[0.5, 1.0, 0.0, 0.0], [0.5, 2.0, 0.0, 0.25], [0.5, 3.0, 0.0, 0.5]]
    assert xgblinear._hyper(-0.5, 0.0, 0.0, 0.0)[0][0] == -0.5          # eta has no sign rule
    with pytest.raises(RuntimeError, match=r"batch sizes differ: \[2, 3\]"):
        xgblinear._hyper([0.1, 0.2], [1.0, 2.0, 3.0], 0.0, 0.0)
    with pytest.raises(ValueError, match="chunk"):
        xgblinear.train(X4, Y4, chunk=0)


FOLD4 = np.array([0, 1, 0, 1])


@pytest.mark.parametrize("kw,msg", [
    (dict(grid=[(1.0, -0.5)]), "alpha"),
    (dict(grid=[(float("nan"), 0.0)]), "lambda_"),
    (dict(grid=[]), "grid"),
    (dict(grid=[(1.0, 0.0, 2.0)]), "grid"),
    (dict(rule="best"), "rule"),
    (dict(fold=np.array([0, 1, 0])), "fold"),
    (dict(fold=np.array([0.0, 1.0, 0.0, 1.0])), "fold"),
    (dict(fold=np.array([0, 2, 0, 2])), "fold 1 has no rows"),
    (dict(fold=np.array([0, 0, 0, 0])), "two folds"),
    (dict(fold=np.array([0, -1, 0, 1])), "fold"),
    (dict(fold=np.array([0, 1, 2, 0]), weight=np.array([1.0, 0.0, 1.0, 1.0])), "fold 1 has no weight for target 0"),
    (dict(fold=np.array([0, 1, 2, 0]), weight=np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, 0.0]]),
          y=np.zeros((2, 4))), "fold 0 has no weight for target 1"),
    (dict(weight=np.array([1.0, 0.0, 1.0, 0.0])), "training rows of fold 0 have no weight"),
    (dict(weight=np.array([1.0, -1.0, 1.0, 1.0])), "weights"),
    (dict(y=np.zeros(5)), "y must be"),
    (dict(eta=float("nan")), "eta"),
    (dict(lambda_bias=-1.0), "lambda_bias"),
    (dict(num_round=0), "num_round"),
])
def test_cv_refuses_before_any_launch(kw, msg):
    args = dict(X=X4, y=Y4, fold=FOLD4, grid=[(1.0, 0.0)])
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        xgblinear.cv(args.pop("X"), args.pop("y"), args.pop("fold"), args.pop("grid"), **args)


def _args(*extra):
    return cli.build_parser(cv=True).parse_args(["--targetIndex", "1", *extra])


def test_cli_refusals():
    with pytest.raises(ValueError, match="n_bootstrap"):
        cli.check_cv_args(_args("--cv", "3", "--n_bootstrap", "2"))
    with pytest.raises(ValueError, match="n_bootstrap"):
        cli.run(_args("--cv", "3", "--n_bootstrap", "2", "--output_dir", "/nonexistent/never/made"))
    with pytest.raises(ValueError, match="at least 2"):
        cli.check_cv_args(_args("--cv", "1"))
    for flags in (("--l2-grid", "1", "10"), ("--l1-grid", "0.5"), ("--cv-only",), ("--cv-rule", "1se")):
        with pytest.raises(ValueError, match="--cv"):
            cli.check_cv_args(_args(*flags))
    cli.check_cv_args(_args())
    cli.check_cv_args(_args("--cv", "5", "--l2-grid", "1", "10", "--cv-rule", "1se", "--cv-only"))
