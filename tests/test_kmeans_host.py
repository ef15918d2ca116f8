"""The host side of the k-means (no GPU): the numpy restatement of the contract (tests/kmeans_ref.py)
against scikit-learn's recorded results (tests/golden/kmeans, written by make_golden_kmeans.py) and,
where it is installed, against scikit-learn itself; ``cluster_and_viz.kmeans_draws``; and the planner
header (expecto_amd/csrc/kmeans_plan.h) built alone into tests/kmeans_plan_driver.cpp, also under the
address and undefined sanitizers.

Equality with sklearn is not guaranteed by construction (a rounding difference can flip a near-tie),
so the inputs are fixed in ``kmeans_ref.INPUTS`` and every case is compared.  Inertia is compared
within n * 2^-52 relative, the worst case of reordering a sum of n non-negative terms."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import kmeans_ref
from conftest import GOLDEN
from expecto_amd import cluster_and_viz

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "kmeans_plan_driver.cpp")
GOLD = os.path.join(GOLDEN, "kmeans")
ALL = [(name, k, n_init, seed) for name, k, n_init in kmeans_ref.CASES for seed in kmeans_ref.SEEDS]
IDS = [kmeans_ref.case_name(*c) for c in ALL]


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLD, "sklearn.npz")) as z:
        return {key: z[key] for key in z.files}


@functools.lru_cache(maxsize=None)
def inputs(name):
    X = kmeans_ref.INPUTS[name]()
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def restated(name, k, n_init, seed):
    return kmeans_ref.fit(inputs(name), k, n_init=n_init, seed=seed)


def test_every_case_is_recorded():
    assert sorted(golden()) == sorted(c + s for c in IDS for s in ("_seeds", "_labels", "_inertia", "_n_iter"))
    for name in kmeans_ref.INPUTS:
        X = inputs(name)
        assert np.array_equal(X, X.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name,k,n_init,seed", ALL, ids=IDS)
def test_restatement_equals_sklearn_golden(name, k, n_init, seed):
    z, case, X = golden(), kmeans_ref.case_name(name, k, n_init, seed), inputs(name)
    first, u = cluster_and_viz.kmeans_draws(seed, X.shape[0], [k], 1)[0][0]      # the right indices need the right stream
    idx, centres = kmeans_ref.plusplus(X, k, first, u)
    assert np.array_equal(idx, z[case + "_seeds"])
    assert np.array_equal(centres, X[idx])
    got = restated(name, k, n_init, seed)
    assert np.array_equal(got["labels"], z[case + "_labels"])
    assert got["n_iter"] == int(z[case + "_n_iter"])
    want = float(z[case + "_inertia"])
    assert abs(got["inertia"] - want) <= X.shape[0] * 2.0 ** -52 * want, (got["inertia"], want)


@pytest.mark.parametrize("name,k,n_init,seed", ALL, ids=IDS)
def test_restatement_equals_sklearn_live(name, k, n_init, seed):
    pytest.importorskip("sklearn")
    from sklearn.cluster import KMeans, kmeans_plusplus
    X = inputs(name)
    got = restated(name, k, n_init, seed)
    if n_init == 1:
        assert np.array_equal(got["seeds"], kmeans_plusplus(np.array(X), k, random_state=seed)[1])
    km = KMeans(k, n_init=n_init, random_state=seed).fit(np.array(X))
    assert np.array_equal(got["labels"], km.labels_) and got["n_iter"] == km.n_iter_
    assert abs(got["inertia"] - km.inertia_) <= X.shape[0] * 2.0 ** -52 * km.inertia_


def test_draws():
    """One stream over the ks in the order given; the restatement's draws; k = 1 draws no uniforms."""
    got = cluster_and_viz.kmeans_draws(5, 40, [3, 1, 9], 2)
    want = kmeans_ref.draws(5, 40, [3, 1, 9], 2)
    rs = np.random.RandomState(5)
    for k, per_g, per_w in zip([3, 1, 9], got, want):
        assert len(per_g) == 2
        for (first, u), (first_w, u_w) in zip(per_g, per_w):
            T = 2 + int(np.log(k))
            assert first == first_w == rs.choice(40, p=np.full(40, 1.0) / 40.0)
            assert u.shape == (k - 1, T) and u.dtype == np.float64
            for c in range(k - 1):
                assert np.array_equal(u[c], rs.uniform(size=T))
            assert np.array_equal(u, u_w.reshape(k - 1, T))
    np.random.seed(0)                       # the reference's stream after its np.random.seed(0)
    first, u = cluster_and_viz.kmeans_draws(0, 40, [4], 1)[0][0]
    assert first == np.random.choice(40, p=np.full(40, 1.0) / 40.0) and np.array_equal(u[0], np.random.uniform(size=3))


def test_reference_run_labels():
    """The reference CLI's recorded clusters (sklearn's float32 route) are the restatement's on the fixture."""
    X = kmeans_ref.cli_reduced(kmeans_ref.CLI_MARKS)[:, :20].astype(np.float64)
    table = pd.read_csv(os.path.join(GOLD, "cli", "all_feature_clusters.tsv"), sep="\t", index_col=0)
    assert table.shape[0] == kmeans_ref.CLI_MARKS
    assert np.array_equal(kmeans_ref.fit(X, 30, seed=0)["labels"], table["cluster"].to_numpy())


def test_restatement_relocation_and_ties():
    """Equal distances go to the lowest centre; empty clusters take the farthest points, the lower index
    on equal dist; a relocated point leaves its old cluster's mean."""
    X = np.array([[0.0], [0.0], [2.0], [2.0], [10.0], [-8.0]])
    C = np.array([[1.0], [1.0], [50.0], [60.0]])
    label, dist = kmeans_ref.e_step(X, C)
    assert label.tolist() == [0] * 6 and dist.tolist() == [1.0, 1.0, 1.0, 1.0, 81.0, 81.0]
    C_new, _ = kmeans_ref.m_step(X, C, label, dist)
    # empties 1, 2, 3 take points 4, 5 (dist 81, index order) and then point 0 (dist 1, lowest index)
    assert C_new.ravel().tolist() == [4.0 / 3.0, 10.0, -8.0, 0.0]
    out = kmeans_ref.lloyd(X, np.array([[3.0]]), 0.0, 300)
    assert out[3] == 2 and out[1].ravel().tolist() == [1.0]


def test_kmeans_refuses_before_the_device():
    X = np.ones((5, 3))
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[1, 2] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            cluster_and_viz.kmeans(Y, 2)
    with pytest.raises(ValueError, match="n_clusters"):
        cluster_and_viz.kmeans(X, 6)
    with pytest.raises(ValueError, match="n_clusters"):
        cluster_and_viz.kmeans(X, 0)
    with pytest.raises(ValueError, match="supported"):
        cluster_and_viz.kmeans(np.ones((4097, 2)), 2)
    with pytest.raises(ValueError, match="n_init"):
        cluster_and_viz.kmeans(X, 2, n_init=0)
    with pytest.raises(ValueError, match="max_iter"):
        cluster_and_viz.kmeans(X, 2, max_iter=0)


# ---- the planner header ------------------------------------------------------------------------

def _cxx():
    return [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]


def run_driver(exe, cases):
    """cases: [(kind, n, d, ld, rows)] -> per case the error text or the tuple of totals."""
    text = ""
    for kind, n, d, ld, rows in cases:
        text += f"{kind} {n} {d} {ld} {len(rows)}\n"
        for r in rows:
            text += " ".join(str(int(v)) for v in list(r) + [0] * (8 - len(r))) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    return [ln[6:] if ln.startswith("error ") else tuple(int(v) for v in ln.split()[1:]) for ln in out]


PLAN_CASES = [
    ("seed", 65, 3, 4, [(3, 1, 2, 0, 0, 0), (2, 5, 2, 4, 3, 3)]),
    ("seed", 2002, 20, 20, [(k, k, 2 + int(np.log(k)), 0, 0, 0) for k in (197,)]),
    ("seed", 65, 3, 3, [(1, 0, 1, 0, 0, 0), (1, 64, 8, 0, 1, 1)]),
    ("lloyd", 65, 3, 4, [(3, 5, 0, 0, 0), (2, 5, 3, 3, 65)]),
    ("lloyd", 4096, 128, 128, [(512, 300, 0, 0, 0)]),
    ("seed", 65, 3, 3, []),
    ("seed", 65, 3, 3, [(0, 0, 1, 0, 0, 0)]),
    ("seed", 65, 3, 3, [(66, 0, 1, 0, 0, 0)]),
    ("seed", 600, 3, 3, [(513, 0, 1, 0, 0, 0)]),
    ("seed", 65, 3, 3, [(2, 65, 1, 0, 0, 0)]),
    ("seed", 65, 3, 3, [(2, 0, 9, 0, 0, 0)]),
    ("seed", 65, 3, 3, [(2, 0, 2, 1, 0, 0)]),
    ("seed", 65, 3, 3, [(2, 0, 2, 0, 0, 0), (2, 0, 2, 2, 1, 2)]),
    ("seed", 65, 3, 2, [(2, 0, 2, 0, 0, 0)]),
    ("seed", 4097, 3, 3, [(2, 0, 2, 0, 0, 0)]),
    ("seed", 65, 129, 129, [(2, 0, 2, 0, 0, 0)]),
    ("lloyd", 65, 3, 3, [(2, 0, 0, 0, 0)]),
    ("lloyd", 65, 3, 3, [(2, 5, 0, 0, 0), (2, 5, 2, 2, 64)]),
    ("lloyd", 65, 3, 3, [(2, 5, 0, 0, 0), (2, 5, 2, 1, 65)]),
]
PLAN_WANT = [
    (3, 2, 6, 5, 5, 0, 0, 8 * 2 * max(4 * 65 * 2, 9 + 65 + 65 + 33)),
    (197, 7, 196 * 7, 197, 197, 0, 0, 8 * max(4 * 2002 * 7, 2 * 3940 + 2002 + 1001)),
    (1, 8, 0, 2, 2, 0, 0, 8 * 2 * 4 * 65 * 8),
    (3, 0, 0, 0, 5, 5, 130, 8 * 2 * max(4 * 65, 9 + 65 + 65 + 33)),
    (512, 0, 0, 0, 512, 512, 4096, 8 * (2 * 65536 + 4096 + 2048)),
    (0, 0, 0, 0, 0, 0, 0, 0),
    "kmeans_plusplus: k must lie in [1, 512]", "kmeans_plusplus: k > n", "kmeans_plusplus: k must lie in [1, 512]",
    "kmeans_plusplus: first outside [0, n)", "kmeans_plusplus: T must lie in [1, 8]",
    "kmeans_plusplus: inconsistent offsets (first not 0, decreasing, or overlapping blocks)",
    "kmeans_plusplus: inconsistent offsets (first not 0, decreasing, or overlapping blocks)",
    "kmeans: row stride ld < d", "kmeans: n must lie in [1, 4096]", "kmeans: d must lie in [1, 128]",
    "kmeans_lloyd: max_iter must lie in [1, 2^31)",
    "kmeans_lloyd: inconsistent offsets (first not 0, decreasing, or overlapping blocks)",
    "kmeans_lloyd: inconsistent offsets (first not 0, decreasing, or overlapping blocks)",
]


def test_plan_driver(tmp_path):
    exe = str(tmp_path / "kmeans_plan_driver")
    subprocess.run(_cxx() + ["-std=c++17", "-O2", "-Wall", SRC, "-o", exe], check=True)
    assert run_driver(exe, PLAN_CASES) == PLAN_WANT


def test_plan_driver_under_sanitizers(tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined and run directly: same output, no report."""
    exe = str(tmp_path / "kmeans_plan_driver_san")
    build = subprocess.run(_cxx() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                                     "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the host compiler has no address/undefined sanitizer runtime: " + build.stderr[-200:])
    assert run_driver(exe, PLAN_CASES) == PLAN_WANT
