"""Silhouette sweep on the device: the kernels of csrc/silhouette.hip through their C entry points,
``interpret_features.silhouette_sweep`` / ``silhouette_samples`` / ``ward_tree(return_condensed=True)``
and the ``--silhouette`` / ``--n_clusters auto`` options of the CLI.

Both kernels run 256 lanes over consecutive points and the square expansion works in 32 x 32 tiles;
the point counts below sit on both sides of 32, 64 and 256.  Outputs lie in pattern-filled buffers
(tests/guarded.py) and the distances inside NaN margins, so a store outside an output or a load
outside the matrix fails the test.  Every comparison with the restatement (tests/silhouette_ref.py)
and with sklearn's recorded bits (tests/golden/silhouette) is bitwise."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import silhouette_ref
import ward_ref
from conftest import GOLDEN
from guarded import Guarded, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
GOLD = os.path.join(GOLDEN, "interpret_features")
SIZES = [2, 3, 63, 64, 65, 129, 257, 600]      # the last two: more than one workgroup of points


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


class Margined64:
    """float64 values on the device with ``margin`` NaNs before and after."""

    def __init__(self, a, margin=64):
        a = np.ascontiguousarray(a, np.float64).ravel()
        host = np.full(margin + a.size + margin, np.nan)
        host[margin:margin + a.size] = a
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin


def csr(lists):
    ptr = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int64)
    flat = np.concatenate([np.asarray(m, np.int32) for m in lists]) if lists else np.empty(0, np.int32)
    return ptr, flat.astype(np.int32)


def hp(a):
    return a.ctypes.data


@functools.lru_cache(maxsize=None)
def points(n):
    X = ward_ref.gamma_points(n, 5, seed=11)
    cond = ward_ref.pdist(X)
    cond.setflags(write=False)
    return cond, silhouette_ref.square(cond, n)


def device_square(lib, cond, n):
    out = Guarded((n, n), np.float64)
    src = Margined64(cond)
    assert lib.expecto_square_distances(src.ptr, n, out.ptr, ST()) == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    return out


def device_node_sums(lib, cond, n, lists, square):
    ptr, members = csr(lists)
    d_ptr, d_members = dev(ptr), dev(members if members.size else np.zeros(1, np.int32))
    src = device_square(lib, cond, n) if square else Margined64(cond)
    S = Guarded((len(lists), n), np.float64)
    st = lib.expecto_silhouette_node_sums(src.ptr, int(square), n, hp(ptr), d_ptr.data_ptr(), d_members.data_ptr(),
                                          len(lists), S.ptr, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    return S.result()


def device_cuts(lib, S, n, sizes, cut_lists, own):
    ptr, active = csr(cut_lists)
    d = [Margined64(S), dev(np.asarray(sizes, np.int32)), dev(ptr), dev(active if active.size else np.zeros(1, np.int32)),
         dev(np.ascontiguousarray(own, np.int32))]
    out = Guarded((len(cut_lists), n), np.float64)
    st = lib.expecto_silhouette_cuts(d[0].ptr, n, len(sizes), d[1].data_ptr(), hp(ptr), d[2].data_ptr(), d[3].data_ptr(),
                                     d[4].data_ptr(), len(cut_lists), out.ptr, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    return out.result()


def node_lists(n):
    """A single point, all but the last point, the first and last point only, a random subset, every
    point, and lengths around the kernel's unroll of 8."""
    rng = np.random.default_rng(n)
    lists = [[0], list(range(n - 1)), [0, n - 1], sorted(rng.choice(n, max(1, n // 3), replace=False).tolist()),
             list(range(n)), [n - 1]]
    lists += [list(range(1, 1 + m)) for m in (7, 8, 9, 17) if 1 + m <= n]
    return lists


@pytest.mark.parametrize("square", [False, True], ids=["condensed", "square"])
@pytest.mark.parametrize("n", SIZES)
def test_node_sums(lib, n, square):
    cond, D = points(n)
    if square:
        assert_bits(device_square(lib, cond, n).result(), D, f"square {n}")
    lists = node_lists(n)
    want = np.stack([silhouette_ref.node_sum(D, m) for m in lists])
    assert_bits(device_node_sums(lib, cond, n, lists, square), want, f"node sums {n}")
    one = device_node_sums(lib, cond, n, lists[2:3], square)          # a node list that is a single node
    assert_bits(one, want[2:3], f"single node {n}")


@pytest.mark.parametrize("n", SIZES[1:])
def test_cuts(lib, n):
    """Every cut of the tree (k = 2 and k = n - 1 among them; at n - 1 all points but two are singletons
    with s = 0) from the restated node sums, against the restated samples."""
    from expecto_amd.interpret_features import plan_sweep
    cond, D = points(n)
    children, _, _ = ward_ref.linkage(cond, n)
    ks = list(range(2, n)) if n <= 129 else [2, 3, 64, n // 2, n - 2, n - 1]
    plan = plan_sweep(children, n, ks)
    lists = [plan.members[plan.node_ptr[v]:plan.node_ptr[v + 1]] for v in range(len(plan.nodes))]
    S = np.stack([silhouette_ref.node_sum(D, m) for m in lists])
    cuts = [plan.active[plan.cut_ptr[c]:plan.cut_ptr[c + 1]] for c in range(len(ks))]
    _, want = silhouette_ref.sweep(children, D, ks)
    got = device_cuts(lib, S, n, plan.sizes, cuts, plan.own)
    assert_bits(got, want, f"cuts {n}")
    assert (got[-1] == 0).sum() >= n - 2 and not np.signbit(got[got == 0]).any()
    # one cut alone, and the device's own node sums feeding the cuts
    assert_bits(device_cuts(lib, S, n, plan.sizes, cuts[:1], plan.own[:1]), want[:1], f"one cut {n}")
    S_dev = device_node_sums(lib, cond, n, lists, square=True)
    assert_bits(device_cuts(lib, S_dev, n, plan.sizes, cuts, plan.own), want, f"sums + cuts {n}")


def test_duplicates_give_zero_samples(lib):
    """The tripled points: where a cut separates duplicates a = b = 0, 0 / 0, s = +0.0."""
    from expecto_amd.interpret_features import plan_sweep
    X = silhouette_ref.triple_points()
    n = X.shape[0]
    cond = ward_ref.pdist(X)
    D = silhouette_ref.square(cond, n)
    children, _, _ = ward_ref.linkage(cond, n)
    ks = list(range(2, n))
    plan = plan_sweep(children, n, ks)
    lists = [plan.members[plan.node_ptr[v]:plan.node_ptr[v + 1]] for v in range(len(plan.nodes))]
    S = device_node_sums(lib, cond, n, lists, square=False)
    got = device_cuts(lib, S, n, plan.sizes, [plan.active[plan.cut_ptr[c]:plan.cut_ptr[c + 1]] for c in range(len(ks))],
                      plan.own)
    z = np.load(os.path.join(GOLDEN, "silhouette", "triples.npz"))
    assert_bits(got, z["samples"], "triples vs sklearn's bits")
    # a pair of duplicates whose third copy is another cluster: a = 0 / 1, b = 0 / 1
    triple = plan.own.reshape(len(ks), n // 3, 3)
    in_pair = (plan.sizes[plan.own] == 2) & np.repeat((triple != triple[:, :, :1]).any(axis=2), 3, axis=1)
    assert in_pair.any() and (got[in_pair] == 0).all() and not np.signbit(got[in_pair]).any()


def test_nothing_to_do(lib):
    """Zero nodes and zero cuts write nothing and succeed, whatever the other pointers are."""
    out = Guarded((4, 8), np.float64)
    assert lib.expecto_silhouette_node_sums(None, 0, 8, None, None, None, 0, out.ptr, ST()) == 0
    assert lib.expecto_silhouette_cuts(None, 8, 3, None, None, None, None, None, 0, out.ptr, ST()) == 0
    torch.cuda.synchronize()
    assert out.untouched()


def test_refusals(lib):
    n = 8
    cond, D = points(64)
    src, out = Margined64(cond), Guarded((4, n), np.float64)
    ok_ptr, members = csr([[0, 1], [2]])
    d_ptr, d_members = dev(ok_ptr), dev(members)
    sums = lambda **k: lib.expecto_silhouette_node_sums(*[k.get(a, v) for a, v in (
        ("dist", src.ptr), ("square", 0), ("n", n), ("host", hp(ok_ptr)), ("ptr", d_ptr.data_ptr()),
        ("members", d_members.data_ptr()), ("n_nodes", 2), ("S", out.ptr))], ST())
    bad = [np.array(v, np.int64) for v in ([1, 2, 3], [0, 2, 1], [0, n + 1, n + 2])]
    for kw, text in (({"n": 1}, "fewer than 2 points"), ({"n": (1 << 20) + 1}, "at most 1048576 points"),
                     ({"n_nodes": -1}, "node count out of range"), ({"dist": None}, "null argument"),
                     ({"S": None}, "null argument"), ({"host": None}, "null argument"),
                     ({"host": hp(bad[0])}, "inconsistent node offsets"), ({"host": hp(bad[1])}, "inconsistent node offsets"),
                     ({"host": hp(bad[2])}, "inconsistent node offsets")):
        assert sums(**kw) == -1, kw
        assert text in lib.expecto_last_error().decode(), kw
    S = Margined64(np.zeros((3, n)))
    sizes, own = dev(np.array([3, 3, 2], np.int32)), dev(np.zeros((1, n), np.int32))
    cut_ok = np.array([0, 2], np.int64)
    d_cut, d_active = dev(cut_ok), dev(np.arange(n, dtype=np.int32))
    cuts = lambda **k: lib.expecto_silhouette_cuts(*[k.get(a, v) for a, v in (
        ("S", S.ptr), ("n", n), ("n_nodes", 3), ("sizes", sizes.data_ptr()), ("host", hp(cut_ok)), ("ptr", d_cut.data_ptr()),
        ("active", d_active.data_ptr()), ("own", own.data_ptr()), ("n_cuts", 1), ("out", out.ptr))], ST())
    badc = [np.array(v, np.int64) for v in ([0, 1], [0, n], [1, 3], [0, 3, 2])]
    for kw, text in (({"n": 1}, "fewer than 2 points"), ({"n": 2}, "fewer than 2 or more than n - 1 clusters"),
                     ({"host": hp(badc[0])}, "fewer than 2 or more than n - 1 clusters"),
                     ({"host": hp(badc[1])}, "fewer than 2 or more than n - 1 clusters"),
                     ({"host": hp(badc[2])}, "inconsistent cut offsets"),
                     ({"host": hp(badc[3]), "n_cuts": 2}, "inconsistent cut offsets"),
                     ({"n_cuts": -1}, "out of range"), ({"own": None}, "null argument"), ({"out": None}, "null argument")):
        assert cuts(**kw) == -1, kw
        assert text in lib.expecto_last_error().decode(), kw
    sq = Guarded((n, n), np.float64)
    for args, text in (((src.ptr, 1, sq.ptr), "fewer than 2 points"), ((None, n, sq.ptr), "null argument"),
                       ((src.ptr, n, None), "null argument"), ((src.ptr, (1 << 20) + 1, sq.ptr), "at most 1048576")):
        assert lib.expecto_square_distances(*args, ST()) == -1
        assert text in lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    assert out.untouched() and sq.untouched()


# ---- Python API ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["gamma", "ties"])
def test_sweep_equals_sklearns_bits(name):
    """All k on gamma_points(70, 33) and tie_points(65, 5): the recorded samples and scores; the same
    from a device tensor as from a numpy array, unsorted ks, and twice the same bits."""
    from expecto_amd.interpret_features import silhouette_sweep, ward_tree
    X = silhouette_ref.INPUTS[name]()
    n = X.shape[0]
    z = np.load(os.path.join(GOLDEN, "silhouette", name + ".npz"))
    ks = [int(k) for k in z["ks"]]
    children, _, cond = ward_tree(X, return_condensed=True)
    before = cond.clone()
    scores, samples = silhouette_sweep(children, cond, n, ks)
    assert scores.dtype == np.float64 and samples.dtype == np.float64
    assert_bits(samples, z["samples"], name + " samples")
    assert_bits(scores, z["scores"], name + " scores")
    assert torch.equal(cond, before)
    again = silhouette_sweep(children, cond.cpu().numpy(), n, ks)
    assert_bits(again[1], samples, "second call, numpy distances")
    assert_bits(again[0], scores, "second call, numpy distances")
    some = [ks[-1], 5, 31, 2]
    got = silhouette_sweep(children, cond, n, some)
    assert_bits(got[1], z["samples"][[k - 2 for k in some]], "unsorted ks")
    assert_bits(got[0], z["scores"][[k - 2 for k in some]], "unsorted ks")


@pytest.mark.parametrize("name", ["gamma", "ties"])
def test_ward_tree_return_condensed(name):
    """test_gpu_cluster.test_ward_tree's trees, with the distances of the restated pdist beside them."""
    from expecto_amd.interpret_features import ward_tree
    X = ward_ref.gamma_points(130, 257) if name == "gamma" else ward_ref.tie_points(64, 6)
    want = ward_ref.pdist(X)
    children, heights, _ = ward_ref.linkage(want, X.shape[0])
    got = ward_tree(X, return_condensed=True)
    assert len(got) == 3 and len(ward_tree(X)) == 2
    assert_bits(got[0], children, "children")
    assert_bits(got[1], heights, "heights")
    assert got[2].is_cuda and got[2].dtype == torch.float64
    assert_bits(got[2].cpu().numpy(), want, "condensed")


def test_silhouette_samples_of_arbitrary_labels():
    from expecto_amd.interpret_features import silhouette_samples
    n = 300
    cond, D = ward_ref.pdist(ward_ref.gamma_points(n, 4, seed=5)), None
    D = silhouette_ref.square(cond, n)
    rng = np.random.default_rng(8)
    for labels in (rng.integers(0, 7, n), np.where(np.arange(n) == 17, -5, 1000), np.arange(n) // 2 * 3,
                   np.minimum(np.arange(n), n - 2).astype(np.int32)):
        got = silhouette_samples(torch.from_numpy(cond).cuda(), labels)
        assert_bits(got, silhouette_ref.samples(D, labels), "arbitrary labels")
    assert_bits(silhouette_samples(cond, labels), got, "numpy distances")


# ---- CLI -------------------------------------------------------------------------------------

def run_cli(capsys, argv):
    from expecto_amd import interpret_features
    capsys.readouterr()
    interpret_features.main([str(a) for a in argv])
    return capsys.readouterr().out


def read(path):
    with open(path, "rb") as f:
        return f.read()


def table(ks, scores):
    return ("n_clusters\tsilhouette_score\n" + "".join(f"{k}\t{float(s)!r}\n" for k, s in zip(ks, scores))).encode()


N_MARKS_UNGROUPED = 40


def cli_case(root, grouped):
    """The golden run's inputs (ward_ref.write_interpret_inputs).  Grouped: all 2,002 marks.  Ungrouped:
    the first 40 marks' ten columns, 400 points (the 20,020 points of all marks cost 5 s of host linkage
    per run and have no affordable restatement).  Returns the argv and the restated (ks, scores)."""
    os.makedirs(root, exist_ok=True)
    x_path, anno_path, exp_path = ward_ref.write_interpret_inputs(root)
    feat = FEATURES_TSV
    X = np.load(x_path)
    if not grouped:
        m = N_MARKS_UNGROUPED
        X = np.ascontiguousarray(X.reshape(-1, 10, ward_ref.INTERPRET_N_MARKS)[:, :, :m].reshape(-1, 10 * m))
        np.save(x_path, X)
        feat = os.path.join(root, "features.tsv")
        with open(FEATURES_TSV) as src, open(feat, "w") as f:
            f.writelines(src.readlines()[:1 + m])
    argv = ["--belugaFeatures", feat, "--targetIndex", 1, "--expFile", exp_path, "--inputFile", x_path, "--annoFile",
            anno_path, "--pseudocount", 0] + (["--grouped"] if grouped else [])
    anno, exp = pd.read_csv(anno_path), pd.read_csv(exp_path)
    train = (~anno["seqnames"].isin(["chrX", "chrY", "chr8"]) & (anno["type"] != "rRNA") & (exp.iloc[:, 1] > 0)).to_numpy()
    Xt = X[train]
    n_marks = X.shape[1] // 10
    P = Xt.reshape(-1, 10, n_marks).transpose(2, 0, 1).reshape(n_marks, -1) if grouped else Xt.T
    cond = ward_ref.pdist(P)
    return argv, P.shape[0], cond


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "ungrouped"])
def test_cli_silhouette(tmp_path_factory, capsys, grouped):
    root = tmp_path_factory.mktemp("sil")
    argv, n, cond = cli_case(str(root / "in"), grouped)
    # without the new options: today's bytes (grouped: the golden files)
    plain = root / "plain"
    stdout = run_cli(capsys, argv + ["--out_dir", plain])
    assert stdout == "Cell type: tissue_b\nClustering complete tree and caching...\n"
    assert not (plain / "silhouette_scores.tsv").exists()
    if grouped:
        assert stdout.encode() == read(os.path.join(GOLD, "stdout.txt"))
        for t in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
            assert read(plain / t) == read(os.path.join(GOLD, t)), t
    # --silhouette 2 40: the restatement's table on the tree the run saved
    z = np.load(plain / "clustering.npz")
    ks = list(range(2, 41))
    scores, _ = silhouette_ref.sweep(z["children"], silhouette_ref.square(cond, n), ks)
    best = int(np.argmax(scores))
    swept = root / "swept"
    stdout = run_cli(capsys, argv + ["--out_dir", swept, "--silhouette", 2, 40])
    assert stdout == ("Cell type: tissue_b\nClustering complete tree and caching...\n"
                      f"Best silhouette score: {float(scores[best])!r} at n_clusters={ks[best]}\n")
    assert read(swept / "silhouette_scores.tsv") == table(ks, scores)
    for t in ("all_feature_clusters.tsv",) + (("cluster_sizes.tsv",) if grouped else ()):     # the default cut is kept
        assert read(swept / t) == read(plain / t), t
    # --n_clusters auto cuts at the argmax: the files of a run given that k
    auto, given = root / "auto", root / "given"
    run_cli(capsys, argv + ["--out_dir", auto, "--silhouette", 2, 40, "--n_clusters", "auto"])
    run_cli(capsys, argv + ["--out_dir", given, "--n_clusters", ks[best], "--clustering_joblib", plain / "clustering.npz"])
    assert read(auto / "all_feature_clusters.tsv") == read(given / "all_feature_clusters.tsv")
    assert len(os.listdir(auto / "clusters")) == ks[best]
    # the saved tree with recomputed distances: the same table; K_MAX is clipped to n - 1
    loaded = root / "loaded"
    stdout = run_cli(capsys, argv + ["--out_dir", loaded, "--silhouette", 2, 40, "--clustering_joblib",
                                     plain / "clustering.npz"])
    assert stdout.startswith(f"Cell type: tissue_b\nLoading clustering model from {plain / 'clustering.npz'}...\nBest ")
    assert read(loaded / "silhouette_scores.tsv") == table(ks, scores)
    if not grouped:
        run_cli(capsys, argv + ["--out_dir", loaded, "--silhouette", n - 3, 10 * n, "--clustering_joblib",
                                plain / "clustering.npz"])
        rows = read(loaded / "silhouette_scores.tsv").decode().splitlines()
        assert [r.split("\t")[0] for r in rows[1:]] == [str(n - 3), str(n - 2), str(n - 1)]
