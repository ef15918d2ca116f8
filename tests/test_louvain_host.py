"""CPU: anchors of the Louvain restatement (tests/louvain_ref.py), which the device is compared with bit
for bit (test_gpu_louvain.py): scikit-learn's neighbours, a set-based Jaccard graph in networkx, networkx's
modularity, local optimality, planted partitions, the ring of cliques, degenerate inputs, and the quality
recorded by tests/golden/make_golden_louvain.py."""
import functools
import json
import os

import networkx as nx
import numpy as np
import pytest

import louvain_ref as ref


def identity(n):
    return np.arange(n, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def blobs_graph():
    X, planted = ref.blobs()
    return ref.symmetrize(*ref.knn_jaccard(X, 8)), planted


@functools.lru_cache(maxsize=None)
def ring():
    return ref.csr_of_networkx(nx.ring_of_cliques(30, 5))


def graph_of(indptr, indices, weights):
    G = nx.Graph()
    G.add_nodes_from(range(len(indptr) - 1))
    for v in range(len(indptr) - 1):
        for e in range(indptr[v], indptr[v + 1]):
            G.add_edge(v, int(indices[e]), weight=float(weights[e]))
    return G


def parts(labels):
    return [set(np.nonzero(labels == c)[0].tolist()) for c in range(int(labels.max()) + 1)]


@pytest.mark.parametrize("n,d,k", [(130, 20, 5), (65, 3, 64), (40, 1, 2)])
def test_neighbours_equal_sklearn(n, d, k):
    from sklearn.neighbors import NearestNeighbors
    X = np.random.RandomState(n).normal(size=(n, d))
    D = np.sort(ref.d2(X), axis=1)
    if k < n:
        gap = float((np.sqrt(D[:, k]) - np.sqrt(D[:, k - 1])).min())
        print("smallest gap between the k-th and the next distance:", gap)
        assert gap > 1e-9          # the premise: no near tie decides a neighbour set
    got = ref.knn(X, k)
    want = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(X).kneighbors(X, return_distance=False)
    assert [set(r) for r in got.tolist()] == [set(r) for r in want.tolist()]
    assert (got[:, 0] == np.arange(n)).all()          # a point is its own first neighbour


def test_jaccard_graph_equals_networkx():
    X = np.random.RandomState(5).normal(size=(90, 4))
    k = 6
    nbr, w = ref.knn_jaccard(X, k)
    sets = [set(r.tolist()) for r in nbr]
    G = nx.Graph()
    G.add_nodes_from(range(90))
    for i in range(90):
        for j in sets[i] - {i}:
            G.add_edge(i, j, weight=len(sets[i] & sets[j]) / len(sets[i] | sets[j]))
    for i in range(90):
        for t in range(k):
            j = int(nbr[i, t])
            assert w[i, t] == (0.0 if j == i else G[i][j]["weight"])
    indptr, indices, weights = ref.symmetrize(nbr, w)
    for i in range(90):
        row = indices[indptr[i]:indptr[i + 1]].tolist()
        assert row == sorted(G[i]) and i not in row
        assert weights[indptr[i]:indptr[i + 1]].tolist() == [G[i][j]["weight"] for j in row]
    from expecto_amd.cluster_and_viz_louvain import symmetrize
    for got, want in zip(symmetrize(nbr, w), (indptr, indices, weights)):
        assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0])
def test_modularity_equals_networkx_and_no_move_gains(gamma):
    for csr in (blobs_graph()[0], ring()):
        n = len(csr[0]) - 1
        res = ref.louvain(*csr, gamma, ref.permutation(0, 0, n))
        assert res["flags"] == 0
        G = graph_of(*csr)
        want = nx.community.modularity(G, parts(res["labels"]), weight="weight", resolution=gamma)
        assert abs(float(res["modularity"]) - want) <= 1e-12
        assert res["n_communities"] == int(res["labels"].max()) + 1
        # labels are numbered by smallest member
        firsts = [int(np.nonzero(res["labels"] == c)[0][0]) for c in range(res["n_communities"])]
        assert firsts == sorted(firsts)
        # on the final aggregated graph no single-node move has a positive gain over staying
        ptr, idx, w = res["graph"]
        k, two_m = ref.degrees(ptr, idx, w)
        assert two_m == res["two_m"]
        comm, D = list(range(len(k))), list(k)
        for v in range(len(k)):
            D[v] = D[v] - k[v]
            g = ref.gains(ptr, idx, w, comm, D, k, v, gamma, two_m)
            assert all(g[c] - g[v] <= 0.0 for c in g), (v, g)
            D[v] = D[v] + k[v]


def test_planted_blobs():
    csr, planted = blobs_graph()
    assert nx.number_connected_components(graph_of(*csr)) == 5
    for seed in range(10):
        res = ref.louvain(*csr, 1.0, ref.permutation(seed, 0, 60))
        assert res["n_communities"] == 5 and ref.same_partition(res["labels"], planted), seed
        assert abs(float(res["modularity"]) - 0.7991) < 5e-5 and res["flags"] == 0


def test_ring_of_cliques():
    csr = ring()
    for seed in range(10):
        hi = ref.louvain(*csr, 4.0, ref.permutation(seed, 0, 150))
        assert hi["n_communities"] == 30 and ref.same_partition(hi["labels"], np.arange(150) // 5)
        lo = ref.louvain(*csr, 1.0, ref.permutation(seed, 0, 150))
        assert lo["n_communities"] < 30 and lo["n_levels"] >= 2
        assert hi["flags"] == 0 and lo["flags"] == 0


def test_degenerate_inputs():
    # k = 1: every point its own only neighbour, no edges
    X = np.random.RandomState(0).normal(size=(7, 3))
    nbr, w = ref.knn_jaccard(X, 1)
    assert (nbr[:, 0] == np.arange(7)).all() and (w == 0).all()
    csr = ref.symmetrize(nbr, w)
    assert csr[1].size == 0
    res = ref.louvain(*csr, 1.0, identity(7))
    assert (res["labels"] == np.arange(7)).all() and res["modularity"] == 0.0
    assert (res["n_communities"], res["n_levels"], res["n_passes"], res["flags"]) == (7, 0, 0, 0)
    # n = 1
    nbr, w = ref.knn_jaccard(np.ones((1, 2)), 1)
    res = ref.louvain(*ref.symmetrize(nbr, w), 1.0, identity(1))
    assert res["labels"].tolist() == [0] and res["flags"] == 0 and res["n_levels"] == 0
    # identical points: ties go to the lower index, so everyone's neighbours are points 0..k-1
    nbr, w = ref.knn_jaccard(np.ones((6, 2)), 3)
    assert (nbr == np.arange(3)).all()
    res = ref.louvain(*ref.symmetrize(nbr, w), 1.0, identity(6))
    assert res["flags"] == 0 and res["n_communities"] >= 1
    # two nodes, one edge
    csr = (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 1.0]))
    res = ref.louvain(*csr, 1.0, identity(2))
    assert res["labels"].tolist() == [0, 0] and res["modularity"] == 0.0
    assert (res["n_communities"], res["n_levels"], res["flags"]) == (1, 1, 0)


def test_bounds_set_their_flags():
    csr = ring()
    perm = ref.permutation(0, 0, 150)
    free = ref.louvain(*csr, 1.0, perm)
    one_pass = ref.louvain(*csr, 1.0, perm, max_passes=1)
    one_level = ref.louvain(*csr, 1.0, perm, max_levels=1)
    assert free["flags"] == 0
    assert one_pass["flags"] & ref.PASS_BOUND
    assert one_level["flags"] == ref.LEVEL_BOUND and one_level["n_levels"] == 1


def test_golden_is_the_restatement_and_quality():
    """The recorded run of the fixture is the restatement's; its best modularity over 8 restarts is within
    networkx's own seed-to-seed spread of networkx's worst, both recorded by make_golden_louvain.py."""
    X = ref.fixture().astype(np.float64)
    assert X.shape == (ref.CLI_MARKS, 20) and np.array_equal(ref.fixture(), ref.make_fixture())
    with np.load(os.path.join(ref.GOLD, "restatement.npz")) as z:
        gold = {key: z[key] for key in z.files}
    nbr, w = ref.knn_jaccard(X, 5)
    assert np.array_equal(nbr, gold["nbr"]) and np.array_equal(w, gold["w"])
    res = ref.louvain(*ref.symmetrize(nbr, w), 1.0, ref.permutation(0, 0, X.shape[0]))
    assert np.array_equal(res["labels"], gold["labels_1.0_0"]) and res["modularity"] == gold["modularity_1.0_0"]
    with open(os.path.join(ref.GOLD, "quality.json")) as f:
        q = json.load(f)
    assert q["ours_per_restart"][0] == float(res["modularity"])
    assert q["ours_best_of_8_restarts"] == max(q["ours_per_restart"])
    assert q["networkx_spread"] == q["networkx_max"] - q["networkx_min"]
    print("ours", q["ours_best_of_8_restarts"], "networkx", q["networkx_min"], q["networkx_median"], q["networkx_max"])
    assert q["ours_best_of_8_restarts"] >= q["networkx_min"] - q["networkx_spread"]
