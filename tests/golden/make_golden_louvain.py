"""Golden files of the Louvain tests, from the restatement (tests/louvain_ref.py), scikit-learn and networkx.

Run from the repo root on a CPU machine (needs pandas, scikit-learn 1.7.2 and networkx 3.4.2; no GPU):
    python tests/golden/make_golden_louvain.py

Writes tests/golden/louvain/:
* ``fixture.npz``: ``X`` float32 [2002, 20], ``louvain_ref.make_fixture()``: a seeded synthetic of the shape
  of the marks' leading SVD coordinates (the k-means goldens hold no coordinates to reuse).
* ``restatement.npz``: the restatement on the fixture at ``k_neighbors = 5``: ``nbr``, ``w``, and for every
  resolution of ``SWEEP`` and restart of ``RESTARTS`` (seed 0) ``labels_<g>_<r>``, ``modularity_<g>_<r>`` and
  ``counters_<g>_<r>`` (n_communities, n_levels, n_passes, flags).
* ``cli.npz`` and ``louvain.json``: what ``python -m expecto_amd.cluster_and_viz_louvain`` writes for the
  fixture with its defaults, from the restatement's labels.  ``cli.npz`` holds the bytes (uint8) of
  ``all_feature_clusters.tsv``, ``cluster_sizes.tsv`` and ``clusters.txt`` (the concatenated
  ``clusters/cluster_<i>.tsv``, each after a ``== cluster_<i>.tsv`` line) under those names: 4,000 lines of
  table that repeat the feature list, kept compressed.
* ``quality.json``: the restatement's best modularity over 8 restarts at resolution 1, and the minimum,
  median and maximum modularity of ``networkx.community.louvain_communities`` over seeds 0..9 on the same
  graph, with their spread.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(GOLD))
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLD)))
import louvain_ref  # noqa: E402

DST = os.path.join(GOLD, "louvain")
FEATURES_TSV = os.path.join(GOLD, "predict_sed", "deepsea_beluga_2002_features.tsv")
SWEEP = (0.5, 1.0, 1.5)
RESTARTS = (0, 1)
QUALITY_RESTARTS = 8
NX_SEEDS = range(10)


def networkx_graph(indptr, indices, weights):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(len(indptr) - 1))
    for v in range(len(indptr) - 1):
        for e in range(indptr[v], indptr[v + 1]):
            G.add_edge(v, int(indices[e]), weight=float(weights[e]))
    return G


def main():
    import networkx as nx

    from expecto_amd import cluster_and_viz_louvain as cvl, predict

    os.makedirs(DST, exist_ok=True)
    X32 = louvain_ref.make_fixture()
    np.savez_compressed(os.path.join(DST, "fixture.npz"), X=X32)
    X = X32.astype(np.float64)
    n = X.shape[0]

    nbr, w = louvain_ref.knn_jaccard(X, 5)
    csr = louvain_ref.symmetrize(nbr, w)
    runs = {}
    for g in SWEEP:
        for r in RESTARTS:
            runs[g, r] = louvain_ref.louvain(*csr, g, louvain_ref.permutation(0, r, n))
    for r in range(QUALITY_RESTARTS):
        if (1.0, r) not in runs:
            runs[1.0, r] = louvain_ref.louvain(*csr, 1.0, louvain_ref.permutation(0, r, n))
    out = dict(nbr=nbr, w=w)
    for g in SWEEP:
        for r in RESTARTS:
            res = runs[g, r]
            out[f"labels_{g}_{r}"] = res["labels"]
            out[f"modularity_{g}_{r}"] = res["modularity"]
            out[f"counters_{g}_{r}"] = np.array([res["n_communities"], res["n_levels"], res["n_passes"], res["flags"]],
                                                np.int32)
    np.savez_compressed(os.path.join(DST, "restatement.npz"), **out)

    # the CLI's files for its defaults: resolution 1, seed 0, one restart
    res = runs[1.0, 0]
    args = argparse.Namespace(resolution=1.0, k_neighbors=5, seed=0)
    features = predict.read_features_table(FEATURES_TSV)
    features['cluster'] = res["labels"]
    work = tempfile.mkdtemp(prefix="expecto_golden_louvain_")
    cvl.write_clusters(work, features, res["n_communities"])
    files = {}
    for name in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
        with open(os.path.join(work, name), "rb") as f:
            files[name] = f.read()
    files["clusters.txt"] = b""
    for i in range(res["n_communities"]):
        with open(os.path.join(work, "clusters", f"cluster_{i}.tsv"), "rb") as src:
            files["clusters.txt"] += f"== cluster_{i}.tsv\n".encode() + src.read()
    shutil.rmtree(work)
    np.savez_compressed(os.path.join(DST, "cli.npz"), **{k: np.frombuffer(v, np.uint8) for k, v in files.items()})
    result = cvl.LouvainResult(res["labels"], float(res["modularity"]), res["n_communities"], res["n_levels"],
                               res["n_passes"], 0, res["flags"])
    with open(os.path.join(DST, "louvain.json"), "w") as f:
        json.dump(cvl.summary(result, args), f, indent=1)
        f.write("\n")

    G = networkx_graph(*csr)
    theirs = [float(nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", resolution=1.0,
                                                                                 seed=s), weight="weight"))
              for s in NX_SEEDS]
    ours = [float(runs[1.0, r]["modularity"]) for r in range(QUALITY_RESTARTS)]
    with open(os.path.join(DST, "quality.json"), "w") as f:
        json.dump({"graph": "fixture, k_neighbors 5, resolution 1", "ours_best_of_8_restarts": max(ours),
                   "ours_per_restart": ours, "networkx_seeds": list(NX_SEEDS), "networkx_min": min(theirs),
                   "networkx_median": float(np.median(theirs)), "networkx_max": max(theirs),
                   "networkx_spread": max(theirs) - min(theirs)}, f, indent=1)
        f.write("\n")
    print("Louvain golden outputs written to", DST)


if __name__ == "__main__":
    main()
