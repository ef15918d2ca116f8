"""Silhouette sweep, host side (no GPU): the numpy restatement (tests/silhouette_ref.py) against
sklearn's recorded bits (tests/golden/silhouette, tests/golden/make_golden_silhouette.py) and, where
it is installed, sklearn itself; the planner ``interpret_features.plan_sweep`` against ``cut_tree``;
and the refusals that must come before any device call.  Every comparison of values is bitwise."""
import functools
import os

import numpy as np
import pytest

import silhouette_ref
import ward_ref
from conftest import GOLDEN
from expecto_amd import interpret_features

NAMES = sorted(silhouette_ref.INPUTS)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, condensed, square D, children, golden file) of a seeded input; shared, read-only."""
    X = silhouette_ref.INPUTS[name]()
    n = X.shape[0]
    cond = ward_ref.pdist(X)
    children, _, _ = ward_ref.linkage(cond, n)
    D = silhouette_ref.square(cond, n)
    for a in (X, cond, D, children):
        a.setflags(write=False)
    return X, cond, D, children, np.load(os.path.join(GOLDEN, "silhouette", name + ".npz"))


@functools.lru_cache(maxsize=None)
def restated_sweep(name):
    _, _, D, children, z = case(name)
    return silhouette_ref.sweep(children, D, [int(k) for k in z["ks"]])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_golden(name):
    X, _, D, children, z = case(name)
    n = X.shape[0]
    assert list(z["ks"]) == list(range(2, n))
    scores, samples = restated_sweep(name)
    assert np.array_equal(bits(samples), bits(z["samples"]))
    assert np.array_equal(bits(scores), bits(z["scores"]))
    for k, lab in zip(z["ks"], z["labels"]):        # the recorded labels are the restated tree's cuts
        assert silhouette_ref.same_partition(ward_ref.cut(children, n, int(k)), lab)
    # one labelling at a time, without the shared node sums
    for c in (0, n // 2, n - 3):
        assert np.array_equal(bits(silhouette_ref.samples(D, z["labels"][c])), bits(z["samples"][c]))
    if name == "triples":
        assert (z["samples"][n // 3 - 2:] == 0).any()       # duplicates split from each other: a = b = 0


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_sklearn(name):
    pytest.importorskip("scipy")
    metrics = pytest.importorskip("sklearn.metrics")
    from scipy.spatial.distance import pdist, squareform
    X, cond, D, children, _ = case(name)
    n = X.shape[0]
    assert np.array_equal(bits(cond), bits(pdist(X)))
    assert np.array_equal(bits(D), bits(squareform(pdist(X))))
    scores, samples = restated_sweep(name)
    for c, k in enumerate(range(2, n)):
        lab = ward_ref.cut(children, n, k)
        assert np.array_equal(bits(samples[c]), bits(metrics.silhouette_samples(D, lab, metric="precomputed")))
        assert bits(scores[c]) == bits(metrics.silhouette_score(D, lab, metric="precomputed"))


@pytest.mark.parametrize("name", ["gamma", "ties"])
def test_planner_cuts_equal_cut_tree(name):
    """Every k in 2..n-1 on a random and on a tie-heavy tree: the plan's clusters are cut_tree's, every
    node's members ascend and are the node's leaves, and a contiguous sweep needs k_min + 2 (k_max - k_min)
    nodes."""
    X, _, _, children, _ = case(name)
    n = X.shape[0]
    ks = list(range(2, n))
    plan = interpret_features.plan_sweep(children, n, ks)
    assert len(plan.nodes) == 2 + 2 * (n - 1 - 2) == len(silhouette_ref.needed_nodes(children, n, ks))
    assert plan.node_ptr[0] == 0 and plan.node_ptr[-1] == len(plan.members)
    assert np.array_equal(np.diff(plan.node_ptr), plan.sizes)
    for v, node in enumerate(plan.nodes):
        m = plan.members[plan.node_ptr[v]:plan.node_ptr[v + 1]]
        assert (np.diff(m) > 0).all()
        assert m.tolist() == sorted(ward_ref.descendants(node, children, n))
    assert np.array_equal(np.diff(plan.cut_ptr), ks)
    for c, k in enumerate(ks):
        labels = interpret_features.cut_tree(children, n, k)
        assert silhouette_ref.same_partition(labels, plan.own[c])
        active = plan.active[plan.cut_ptr[c]:plan.cut_ptr[c + 1]]
        assert sorted(active.tolist()) == sorted(set(plan.own[c].tolist())) and len(active) == k
        for v in active:                          # the row that owns a point lists it
            m = plan.members[plan.node_ptr[v]:plan.node_ptr[v + 1]]
            assert (plan.own[c][m] == v).all()


def test_planner_node_count_of_an_inner_range():
    _, _, _, children, _ = case("gamma")
    plan = interpret_features.plan_sweep(children, 70, list(range(7, 31)))
    assert len(plan.nodes) == 7 + 2 * (30 - 7)


def test_planner_unsorted_and_sparse_ks():
    _, _, _, children, _ = case("ties")
    n = 65
    ks = [40, 3, 64, 17, 2]
    plan = interpret_features.plan_sweep(children, n, ks)
    assert len(plan.nodes) == len(silhouette_ref.needed_nodes(children, n, ks))
    assert np.array_equal(np.diff(plan.cut_ptr), ks)
    for c, k in enumerate(ks):
        assert silhouette_ref.same_partition(interpret_features.cut_tree(children, n, k), plan.own[c])
    full = interpret_features.plan_sweep(children, n, list(range(2, n)))
    assert set(plan.nodes.tolist()) <= set(full.nodes.tolist())


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library or of a device tensor fails the test."""
    from expecto_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(interpret_features, "_run_plan", refuse)


def test_refusals_come_before_the_device(no_device):
    _, cond, _, children, _ = case("gamma")
    n = 70
    for ks in ([1, 2], [2, n], [0], [-3]):
        with pytest.raises(ValueError, match="Valid values are 2 to n_samples - 1 = 69"):
            interpret_features.silhouette_sweep(children, cond, n, ks)
    with pytest.raises(ValueError, match="duplicate n_clusters"):
        interpret_features.silhouette_sweep(children, cond, n, [5, 9, 5])
    with pytest.raises(TypeError):
        interpret_features.silhouette_sweep(children, cond, n, [2.5])
    for bad in (np.nan, np.inf):
        c = cond.copy()
        c[1234] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            interpret_features.silhouette_sweep(children, c, n, [2, 3])
        with pytest.raises(ValueError, match="NaN or infinity"):
            interpret_features.silhouette_samples(c, np.arange(n) % 3)
    with pytest.raises(ValueError, match="2415 distances"):
        interpret_features.silhouette_sweep(children, cond[:-1], n, [2])
    for labels, count in ((np.zeros(n, np.int64), 1), (np.arange(n), n)):      # sklearn's wording
        with pytest.raises(ValueError, match=rf"Number of labels is {count}\. Valid values are 2 to n_samples - 1 "
                                             rf"\(inclusive\)"):
            interpret_features.silhouette_samples(cond, labels)
    with pytest.raises(ValueError, match="integer"):
        interpret_features.silhouette_samples(cond, np.zeros(n))
    with pytest.raises(ValueError, match="not a merge tree"):
        interpret_features.plan_sweep(children[::-1], n, [2])


def test_cli_refusals_come_before_the_device(tmp_path, no_device, monkeypatch):
    """--n_clusters auto without --silhouette, and a K_MIN outside 2..K_MAX, end the run before the tree."""
    monkeypatch.setattr(interpret_features, "ward_tree", lambda *a, **k: pytest.fail("the tree was computed"))
    feat = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
    x_path, anno_path, exp_path = ward_ref.write_interpret_inputs(str(tmp_path))
    argv = ["--grouped", "--belugaFeatures", feat, "--targetIndex", "1", "--expFile", exp_path, "--inputFile", x_path,
            "--annoFile", anno_path, "--pseudocount", "0", "--out_dir", str(tmp_path / "out")]
    with pytest.raises(ValueError, match="--n_clusters auto needs --silhouette"):
        interpret_features.main(argv + ["--n_clusters", "auto"])
    for k_min, k_max in ((1, 40), (41, 40), (2002, 5000)):
        with pytest.raises(ValueError, match="K_MIN must be at least 2"):
            interpret_features.main(argv + ["--silhouette", str(k_min), str(k_max)])
    args = interpret_features.build_parser().parse_args(argv)
    assert args.silhouette is None and args.n_clusters is None
    assert interpret_features.build_parser().parse_args(argv + ["--n_clusters", "7"]).n_clusters == 7


def test_argmax_takes_the_first_maximum(tmp_path, monkeypatch, capsys):
    """Tied scores: --n_clusters auto cuts at the first maximum, np.argmax(scores) + K_MIN."""
    tied = np.array([0.25, 0.5, 0.125, 0.5, 0.5])
    calls = {}

    def fake_sweep(children, condensed, n_leaves, ks):
        calls["ks"] = list(ks)
        return tied, np.zeros((len(ks), n_leaves))
    X, _, _, children, _ = case("ties")
    n = X.shape[0]
    monkeypatch.setattr(interpret_features, "silhouette_sweep", fake_sweep)
    monkeypatch.setattr(interpret_features, "device_points", lambda *a, **k: None)
    monkeypatch.setattr(interpret_features, "pairwise_condensed", lambda *a, **k: None)
    monkeypatch.setattr(interpret_features, "training_rows", lambda args: np.zeros((4, 10 * n)))
    feat = tmp_path / "features.tsv"
    with open(os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")) as src, open(feat, "w") as f:
        f.writelines(src.readlines()[:1 + n])
    np.savez(tmp_path / "tree.npz", children=children, distances=np.zeros(n - 1), n_leaves=n)
    out = tmp_path / "out"
    interpret_features.main(["--grouped", "--belugaFeatures", str(feat), "--out_dir", str(out), "--clustering_joblib",
                             str(tmp_path / "tree.npz"), "--silhouette", "4", "8", "--n_clusters", "auto"])
    assert calls["ks"] == [4, 5, 6, 7, 8]
    assert "Best silhouette score: 0.5 at n_clusters=5\n" in capsys.readouterr().out
    with open(out / "silhouette_scores.tsv") as f:
        assert f.read() == "n_clusters\tsilhouette_score\n4\t0.25\n5\t0.5\n6\t0.125\n7\t0.5\n8\t0.5\n"
    assert len(os.listdir(out / "clusters")) == 5
