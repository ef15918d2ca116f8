"""Louvain on the device: the kernels of csrc/louvain.hip through their C entry points,
``cluster_and_viz_louvain.louvain_sweep`` and the CLI.

``expecto_knn_jaccard`` runs one wave per point, ``expecto_louvain`` one wave per problem; a row of the
graph longer than the wave's 64 lanes takes another path of the search, which the star graph reaches.
Outputs lie in pattern-filled buffers (tests/guarded.py) and X inside NaN margins with NaN row padding
(``ld > d``), so a store outside an output or a load outside the matrix fails the test.  Every comparison
with the restatement (tests/louvain_ref.py) is bitwise."""
import functools
import json
import os

import networkx as nx
import numpy as np
import pytest
import torch

import louvain_ref as ref
from conftest import GOLDEN
from guarded import Guarded, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


class Rows64:
    """float64 [n, d] on the device with row stride ld; NaN padding, NaN margins before and after."""

    def __init__(self, X, ld, margin=64):
        X = np.asarray(X, np.float64)
        n, d = X.shape
        host = np.full(margin + n * ld + margin, np.nan)
        host[margin:margin + n * ld].reshape(n, ld)[:, :d] = X
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin
        self.n, self.d, self.ld = n, d, ld


def knn_device(lib, X, k):
    n, d = X.shape
    src = Rows64(X, d + 3)
    nbr, w = Guarded((n, k), np.int32), Guarded((n, k), np.float64)
    st = lib.expecto_knn_jaccard(src.ptr, n, d, src.ld, k, nbr.ptr, w.ptr, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    return nbr.result(), w.result()


def louvain_device(lib, csr, gammas, perms, max_passes=100, max_levels=32):
    indptr, indices, weights = csr
    n, nnz, P = len(indptr) - 1, len(indices), len(gammas)
    perms = np.ascontiguousarray(perms, np.int32).reshape(P, n)
    d_ptr, d_g, d_perm = dev(np.asarray(indptr, np.int32)), dev(np.asarray(gammas, np.float64)), dev(perms)
    d_idx = dev(np.concatenate([np.asarray(indices, np.int32), np.zeros(1, np.int32)]))
    d_w = dev(np.concatenate([np.asarray(weights, np.float64), np.full(1, np.nan)]))
    labels, mod, counters = Guarded((P, n), np.int32), Guarded((P,), np.float64), Guarded((P, 4), np.int32)
    nbytes = int(lib.expecto_louvain_workspace(n, nnz, P))
    assert nbytes > 0
    ws = Guarded((nbytes // 8,), np.float64)
    st = lib.expecto_louvain(d_ptr.data_ptr(), d_idx.data_ptr(), d_w.data_ptr(), n, nnz, P, d_g.data_ptr(),
                             d_perm.data_ptr(), max_passes, max_levels, labels.ptr, mod.ptr, counters.ptr, ws.ptr,
                             nbytes, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    ws.result()
    return labels.result(), mod.result(), counters.result()


def assert_louvain(lib, csr, gammas, perms, what, **bounds):
    """The device's problems equal the restatement's, bit for bit; returns the restatement's results."""
    labels, mod, counters = louvain_device(lib, csr, gammas, perms, **bounds)
    want = [ref.louvain(*csr, g, p, **bounds) for g, p in zip(gammas, perms)]
    for p, r in enumerate(want):
        assert_bits(labels[p], r["labels"], f"{what} problem {p} labels")
        assert_bits(mod[p], np.float64(r["modularity"]), f"{what} problem {p} modularity")
        assert counters[p].tolist() == [r["n_communities"], r["n_levels"], r["n_passes"], r["flags"]], (what, p)
    return want


@functools.lru_cache(maxsize=None)
def points(n, d):
    X = np.random.RandomState(100 * n + d).normal(size=(n, d)).astype(np.float32).astype(np.float64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def ring():
    return ref.csr_of_networkx(nx.ring_of_cliques(30, 5))


def star_points():
    """A centre and 100 points along the axes of 100 dimensions, at distances 1.0 .. 1.099 from it: any two
    of them are further apart than either is from the centre, so the centre's row of the graph has 100
    entries."""
    return np.vstack([np.zeros((1, 100)), np.diag(1.0 + 0.001 * np.arange(100))])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_knn_jaccard_shapes(lib, n):
    for d in (1, 20, 128):
        X = points(n, d)
        D = ref.d2(X)
        for k in (1, 2, 5, 64):
            if k <= n:
                nbr, w = knn_device(lib, X, k)
                want = np.argsort(D, axis=1, kind="stable")[:, :k].astype(np.int32)
                assert_bits(nbr, want, f"n={n} d={d} k={k} nbr")
                assert_bits(w, ref.jaccard(want), f"n={n} d={d} k={k} w")


def test_knn_jaccard_duplicates_and_star(lib):
    X = np.repeat(points(33, 3), 3, axis=0)[np.random.RandomState(1).permutation(99)]      # every row three times
    for k in (2, 3, 7):
        nbr, w = knn_device(lib, X, k)
        want = ref.knn(X, k)
        assert (ref.d2(X)[np.arange(99), want[:, 1]] == 0).all()
        assert_bits(nbr, want, f"duplicates k={k} nbr")
        assert_bits(w, ref.jaccard(want), f"duplicates k={k} w")
    X = np.ones((70, 4))
    nbr, _ = knn_device(lib, X, 5)
    assert (nbr == np.arange(5)).all()
    X = star_points()
    nbr, w = knn_device(lib, X, 3)
    want = ref.knn(X, 3)
    assert (want[1:, 1] == 0).all()
    assert_bits(nbr, want, "star nbr")
    assert_bits(w, ref.jaccard(want), "star w")


def test_louvain_ring_of_cliques(lib):
    """3 resolutions x 3 orders in one launch; gamma = 1 aggregates twice, gamma = 4 keeps the cliques."""
    gammas = np.repeat([0.5, 1.0, 4.0], 3)
    perms = [ref.permutation(0, r, 150) for r in range(3)] * 3
    want = assert_louvain(lib, ring(), gammas, perms, "ring")
    assert all(r["n_communities"] == 30 for r in want[6:]) and all(r["n_levels"] >= 2 for r in want[3:6])


def test_louvain_star_blobs_and_edgeless(lib):
    X = star_points()
    csr = ref.symmetrize(*ref.knn_jaccard(X, 3))
    assert csr[0][1] - csr[0][0] == 100          # longer than a wave
    assert_louvain(lib, csr, [1.0, 0.3, 2.0], [ref.permutation(0, r, 101) for r in range(3)], "star")
    # a hand-made star with unequal weights: the long row decides moves
    G = nx.star_graph(80)
    for v in range(1, 81):
        G[0][v]["weight"] = 1.0 + (v % 7) / 8
    for v in range(1, 80):
        G.add_edge(v, v + 1, weight=0.75)
    assert_louvain(lib, ref.csr_of_networkx(G), [1.0, 0.1], [ref.permutation(3, r, 81) for r in range(2)], "weighted star")
    Xb, planted = ref.blobs()
    want = assert_louvain(lib, ref.symmetrize(*ref.knn_jaccard(Xb, 8)), [1.0] * 3,
                          [ref.permutation(s, 0, 60) for s in range(3)], "blobs")
    assert all(ref.same_partition(r["labels"], planted) for r in want)
    edgeless = (np.zeros(8, np.int32), np.zeros(0, np.int32), np.zeros(0))
    labels, mod, counters = louvain_device(lib, edgeless, [1.0, 2.0], [ref.permutation(0, r, 7) for r in range(2)])
    assert (labels == np.arange(7)).all() and (mod == 0).all() and counters.tolist() == [[7, 0, 0, 0]] * 2
    two = (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 1.0]))
    assert_louvain(lib, two, [1.0], [np.arange(2)], "two nodes")
    one = (np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert_louvain(lib, one, [1.0], [np.arange(1)], "one node")


def test_louvain_bounds_and_batches(lib):
    perm = ref.permutation(0, 0, 150)
    want = assert_louvain(lib, ring(), [1.0], [perm], "max_passes=1", max_passes=1)
    assert want[0]["flags"] & ref.PASS_BOUND
    want = assert_louvain(lib, ring(), [1.0], [perm], "max_levels=1", max_levels=1)
    assert want[0]["flags"] == ref.LEVEL_BOUND
    # P = 33: each problem alone gives the bits it gives in the batch
    gammas = 0.25 + 0.125 * np.arange(33)
    perms = [ref.permutation(7, r, 150) for r in range(33)]
    labels, mod, counters = louvain_device(lib, ring(), gammas, perms)
    for p in (0, 16, 32):
        alone = louvain_device(lib, ring(), gammas[p:p + 1], perms[p:p + 1])
        assert_bits(alone[0][0], labels[p], f"problem {p} alone")
        assert_bits(alone[1][0], mod[p], f"problem {p} alone")
        r = ref.louvain(*ring(), gammas[p], perms[p])
        assert_bits(labels[p], r["labels"], f"problem {p}")
        assert_bits(mod[p], np.float64(r["modularity"]), f"problem {p}")
        assert counters[p].tolist() == [r["n_communities"], r["n_levels"], r["n_passes"], r["flags"]]


def test_refusals(lib):
    X = points(65, 3)
    src = Rows64(X, 4)
    nbr, w = Guarded((65, 64), np.int32), Guarded((65, 64), np.float64)

    def knn(**kw):
        a = dict(X=src.ptr, n=65, d=3, ld=4, k=5, nbr=nbr.ptr, w=w.ptr)
        a.update(kw)
        return lib.expecto_knn_jaccard(*a.values(), ST())

    for kw, text in ((dict(k=65), "k must lie"), (dict(n=4, k=5), "k > n"), (dict(k=0), "k must lie"),
                     (dict(n=4097), "n must lie"), (dict(d=129), "d must lie"), (dict(ld=2), "ld < d"),
                     (dict(X=None), "null argument"), (dict(nbr=None), "null argument")):
        assert knn(**kw) == -1, kw
        assert text in lib.expecto_last_error().decode(), (kw, text)

    indptr, indices, weights = ring()
    n, nnz = 150, len(indices)
    d_ptr, d_idx, d_w = dev(indptr), dev(indices), dev(weights)
    d_g, d_perm = dev(np.ones(2)), dev(np.stack([ref.permutation(0, r, n) for r in range(2)]))
    labels, mod, counters = Guarded((2, n), np.int32), Guarded((2,), np.float64), Guarded((2, 4), np.int32)
    nbytes = int(lib.expecto_louvain_workspace(n, nnz, 2))
    ws = Guarded((nbytes // 8,), np.float64)

    def louvain(**kw):
        a = dict(ptr=d_ptr.data_ptr(), idx=d_idx.data_ptr(), w=d_w.data_ptr(), n=n, nnz=nnz, P=2, g=d_g.data_ptr(),
                 perm=d_perm.data_ptr(), passes=100, levels=32, labels=labels.ptr, mod=mod.ptr, counters=counters.ptr,
                 ws=ws.ptr, nbytes=nbytes)
        a.update(kw)
        return lib.expecto_louvain(*a.values(), ST())

    for kw, text in ((dict(nbytes=nbytes - 1), "workspace too small"), (dict(n=4097), "n must lie"),
                     (dict(n=0), "n must lie"), (dict(nnz=-1), "nnz must lie"), (dict(P=-1), "problem count"),
                     (dict(passes=0), "max_passes"), (dict(levels=65), "max_levels"), (dict(ptr=None), "null argument"),
                     (dict(labels=None), "null argument"), (dict(ws=None), "null argument")):
        assert louvain(**kw) == -1, kw
        assert text in lib.expecto_last_error().decode(), (kw, text)
    assert lib.expecto_louvain_workspace(4097, 10, 1) == 0 and lib.expecto_louvain_workspace(10, -1, 1) == 0
    assert louvain(P=0) == 0
    torch.cuda.synchronize()
    for g in (nbr, w, labels, mod, counters, ws):
        assert g.untouched()
    # a graph the device finds malformed is passed over with its flag; the good one does run
    bad = indices.copy()
    bad[7] = n
    d_bad = dev(bad)
    assert louvain(idx=d_bad.data_ptr()) == 0
    torch.cuda.synchronize()
    assert labels.untouched() and counters.result().tolist() == [[0, 0, 0, ref.BAD_GRAPH]] * 2
    assert louvain() == 0
    torch.cuda.synchronize()
    assert counters.result()[:, 3].tolist() == [0, 0]


# ---- Python API and CLI ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(ref.GOLD, "restatement.npz")) as z:
        return {key: z[key] for key in z.files}


def test_sweep_equals_restatement():
    from expecto_amd import cluster_and_viz_louvain as cvl
    X, z = ref.fixture(), golden()
    nbr, w = cvl.knn_graph(X, 5)
    assert_bits(nbr, z["nbr"], "nbr")
    assert_bits(w, z["w"], "w")
    for got, want in zip(cvl.symmetrize(nbr, w), ref.symmetrize(z["nbr"], z["w"])):
        assert_bits(got, want, "csr")
    gammas = (0.5, 1.0, 1.5)
    timings = {}
    swept = cvl.louvain_sweep(X, 5, gammas, n_init=2, seed=0, timings=timings)
    assert set(timings) == {"graph_ms", "symmetrize_ms", "louvain_ms"}
    for g, res in zip(gammas, swept):
        mods = [float(z[f"modularity_{g}_{r}"]) for r in (0, 1)]
        assert res.restart == int(np.argmax(mods))          # the first maximum
        r = res.restart
        assert_bits(res.labels, z[f"labels_{g}_{r}"], f"gamma={g} labels")
        assert res.modularity == mods[r]
        assert [res.n_communities, res.n_levels, res.n_passes, res.flags] == z[f"counters_{g}_{r}"].tolist()
    one = cvl.louvain(X, 5, 1.0, seed=1)          # seed 1, restart 0 is seed 0's restart 1
    assert_bits(one.labels, z["labels_1.0_1"], "seed 1")
    assert one.restart == 0
    with pytest.raises(ValueError, match="k_neighbors"):
        cvl.louvain(np.ones((5, 3)), 6)
    with pytest.raises(ValueError, match="NaN or infinity"):
        cvl.louvain(np.full((5, 3), np.nan), 2)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_equals_restatement(tmp_path, capsys):
    from expecto_amd import cluster_and_viz_louvain as cvl, predict_by_cluster
    src = tmp_path / "in"
    src.mkdir()
    np.save(src / "tf_idf_reduced_100.npy", ref.fixture())
    with np.load(os.path.join(ref.GOLD, "cli.npz")) as z:
        gold = {name: z[name].tobytes() for name in z.files}
    argv = [str(src), "--belugaFeatures", FEATURES_TSV]

    def check_cluster_files(out):
        for name in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
            assert read(out / name) == gold[name], name
        k = len(os.listdir(out / "clusters"))
        clusters = b"".join(f"== cluster_{i}.tsv\n".encode() + read(out / "clusters" / f"cluster_{i}.tsv") for i in range(k))
        assert clusters == gold["clusters.txt"]
        with open(out / "louvain.json") as f, open(os.path.join(ref.GOLD, "louvain.json")) as g:
            got, want = json.load(f), json.load(g)
        assert got == want and k == want["n_clusters"]

    cvl.main(argv + ["-o", str(tmp_path / "out")])
    check_cluster_files(tmp_path / "out")
    assert not (tmp_path / "out" / "resolution_sweep.tsv").exists()
    ids, members = predict_by_cluster.feature_clusters(str(tmp_path / "out" / "all_feature_clusters.tsv"), ref.CLI_MARKS)
    assert sum(len(m) for m in members) == ref.CLI_MARKS and ids == list(range(len(ids)))
    # the sweep: its table beside the same cluster files
    cvl.main(argv + ["-o", str(tmp_path / "swept"), "--resolution_sweep", "0.5", "1.6", "0.5"])
    check_cluster_files(tmp_path / "swept")
    z = golden()
    want = "resolution\tn_clusters\tmodularity\trestart\n" + "".join(
        f"{g!r}\t{int(z[f'counters_{g}_0'][0])}\t{float(z[f'modularity_{g}_0'])!r}\t0\n" for g in (0.5, 1.0, 1.5))
    assert read(tmp_path / "swept" / "resolution_sweep.tsv") == want.encode()
    with pytest.raises(ValueError, match="2002 rows"):
        cvl.main(argv + ["--no_tf_features", "-o", str(tmp_path / "bad")])
