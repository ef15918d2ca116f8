"""The host half of the Ward clustering (expecto_amd/csrc/ward_linkage.h, interpret_features.cut_tree
and features_grouped), without a GPU.  The header is built with the host compiler alone into
tests/ward_linkage_driver.cpp, as test_seg_plan.py builds the planner; its trees are compared bit for
bit with the numpy restatement (tests/ward_ref.py) and, where they are installed, with scipy's
``ward`` and sklearn's ``AgglomerativeClustering``."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import ward_ref
from expecto_amd import interpret_features

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "ward_linkage_driver.cpp")

CASES = {f"gamma-{n}x{d}": ("gamma", n, d) for n, d in ((2, 1), (3, 5), (37, 53), (130, 257))}
CASES.update({f"ties-{n}x{d}": ("ties", n, d) for n, d in ((40, 3), (64, 6))})


@functools.lru_cache(maxsize=None)
def points(name):
    kind, n, d = CASES[name]
    X = ward_ref.gamma_points(n, d) if kind == "gamma" else ward_ref.tie_points(n, d)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference(name):
    """(condensed, children, heights, sizes) of the restatement, computed once."""
    X = points(name)
    cond = ward_ref.pdist(X)
    out = (cond,) + ward_ref.linkage(cond, X.shape[0])
    for a in out:
        a.setflags(write=False)
    return out


def _cxx():
    return [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ward") / "ward_linkage_driver")
    subprocess.run(_cxx() + ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", SRC, "-o", exe], check=True)
    return exe


def run_driver(exe, cases):
    """cases: [(n, condensed)] -> per case (children, heights, sizes) or the error text."""
    text = "".join(f"{n}\n" + " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in cond) + "\n"
                   for n, cond in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    res, cur = [], None
    for ln in out.splitlines():
        word, _, rest = ln.partition(" ")
        if word == "case":
            cur = []
        elif word == "error":
            cur = rest
        elif word == "merge":
            a, b, h, s = rest.split()
            cur.append((int(a), int(b), float.fromhex(h), int(s)))
        elif word == "end":
            if isinstance(cur, list):
                m = len(cur)
                cur = (np.array([r[:2] for r in cur], np.int64).reshape(m, 2), np.array([r[2] for r in cur], np.float64),
                       np.array([r[3] for r in cur], np.int64))
            res.append(cur)
    assert len(res) == len(cases)
    return res


def assert_same_tree(got, want, what):
    for g, w, part in zip(got, want, ("children", "heights", "sizes")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, part)
        if g.dtype.kind == "f":
            assert np.array_equal(g.view(np.uint64), np.asarray(w, np.float64).view(np.uint64)), (what, part)
        else:
            assert np.array_equal(g, w), (what, part)


@pytest.mark.parametrize("name", list(CASES))
def test_driver_equals_restatement(driver, name):
    cond, *want = reference(name)
    got, = run_driver(driver, [(points(name).shape[0], cond)])
    assert_same_tree(got, want, name)


def test_ties_are_tie_heavy():
    """The tie cases do hold zero distances and many merges at a height another merge has."""
    for name in ("ties-40x3", "ties-64x6"):
        cond, _, heights, _ = reference(name)
        assert (cond == 0).sum() >= 2
        assert len(heights) - len(np.unique(heights)) >= 20, name


@pytest.mark.parametrize("name", list(CASES))
def test_scipy_ward_bitwise(driver, name):
    pytest.importorskip("scipy")
    from scipy.cluster.hierarchy import ward
    from scipy.spatial.distance import pdist
    X = points(name)
    cond, *want = reference(name)
    assert np.array_equal(pdist(X).view(np.uint64), cond.view(np.uint64))
    Z = ward(X)
    scipy_tree = (Z[:, :2].astype(np.int64), Z[:, 2], Z[:, 3].astype(np.int64))
    assert_same_tree(want, scipy_tree, name + " restatement vs scipy")
    got, = run_driver(driver, [(X.shape[0], cond)])
    assert_same_tree(got, scipy_tree, name + " driver vs scipy")


@pytest.mark.parametrize("name", list(CASES))
def test_cut_tree_equals_restatement(name):
    _, children, _, _ = reference(name)
    n = points(name).shape[0]
    for k in sorted({1, 2, 4, 7, 10, n}):
        if k <= n:
            assert np.array_equal(interpret_features.cut_tree(children, n, k), ward_ref.cut(children, n, k)), (name, k)


@pytest.mark.parametrize("name", list(CASES))
def test_cut_tree_equals_sklearn(name):
    pytest.importorskip("scipy")
    pytest.importorskip("sklearn")
    from sklearn.cluster import AgglomerativeClustering
    X = points(name)
    _, children, _, _ = reference(name)
    n = X.shape[0]
    for k in sorted({2, 4, 7, 10, n}):
        if k > n:
            continue
        model = AgglomerativeClustering(n_clusters=k).fit(X)
        assert np.array_equal(model.children_, children), (name, k)
        got = interpret_features.cut_tree(children, n, k)
        assert got.dtype == np.int64
        assert np.array_equal(got, model.labels_), (name, k)


def test_cut_tree_refusals():
    _, children, _, _ = reference("gamma-37x53")
    with pytest.raises(ValueError, match="more clusters than samples"):
        interpret_features.cut_tree(children, 37, 38)
    with pytest.raises(ValueError, match="children of shape"):
        interpret_features.cut_tree(children, 36, 2)


def test_linkage_refusals(driver):
    nan = np.array([1.0, np.nan, 2.0])
    inf = np.array([np.inf, np.inf, 1.0])     # point 0 has no neighbour at a finite distance
    got = run_driver(driver, [(1, np.empty(0)), (0, np.empty(0)), (3, nan), (3, inf)])
    assert got == ["ward linkage needs at least 2 points", "ward linkage needs at least 2 points",
                   "ward linkage: NaN in the distance matrix",
                   "ward linkage: a cluster has no neighbour at a finite distance"]
    for n, cond, text in ((1, np.empty(0), "at least 2 points"), (3, nan, "NaN in the distance matrix")):
        with pytest.raises(ValueError, match=text):
            ward_ref.linkage(cond, n)


def test_ward_tree_refuses_before_the_device():
    """Too few points, a NaN or an infinity is a ValueError, as sklearn's; raised before any device call."""
    with pytest.raises(ValueError, match="at least 2 are required"):
        interpret_features.ward_tree(np.ones((1, 4)))
    for bad in (np.nan, np.inf):
        X = np.ones((3, 4))
        X[1, 2] = bad
        with pytest.raises(ValueError, match="contains NaN or infinity"):
            interpret_features.ward_tree(X)
    with pytest.raises(ValueError, match="2-D"):
        interpret_features.ward_tree(np.ones(5))


def test_features_grouped():
    """Against the reference's expression (interpret_features_grouped.py:73) on a (12, 70) matrix."""
    n_marks = 7
    X_train = np.random.default_rng(5).normal(size=(12, 10 * n_marks))
    want = X_train.T.reshape(10, n_marks, -1).transpose(1, 2, 0).reshape(n_marks, -1)
    got = interpret_features.features_grouped(X_train, n_marks)
    assert got.shape == (7, 120) and np.array_equal(got, want)
    for f, g, k in ((0, 0, 0), (3, 5, 9), (6, 11, 4)):
        assert got[f, g * 10 + k] == X_train[g, k * n_marks + f]
    import torch
    assert np.array_equal(interpret_features.features_grouped(torch.from_numpy(X_train), n_marks).numpy(), want)
    with pytest.raises(ValueError, match="expected"):
        interpret_features.features_grouped(X_train, 8)


def test_load_tree_round_trip(tmp_path):
    _, children, heights, _ = reference("ties-40x3")
    path = str(tmp_path / "clustering.npz")
    np.savez(path, children=children, distances=heights, n_leaves=40)
    c, h, n = interpret_features.load_tree(path)
    assert n == 40 and np.array_equal(c, children) and np.array_equal(h, heights)


def test_driver_under_sanitizers(tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined and run directly on every case,
    the refusals included: same output, no report."""
    exe = str(tmp_path / "ward_linkage_driver_san")
    build = subprocess.run(_cxx() + ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                     "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the host compiler has no address/undefined sanitizer runtime: " + build.stderr[-200:])
    cases = [(points(name).shape[0], reference(name)[0]) for name in CASES]
    got = run_driver(exe, cases + [(1, np.empty(0)), (3, np.array([1.0, np.nan, 2.0]))])
    for name, g in zip(CASES, got):
        assert_same_tree(g, reference(name)[1:], name + " under sanitizers")
    assert got[-2:] == ["ward linkage needs at least 2 points", "ward linkage: NaN in the distance matrix"]
