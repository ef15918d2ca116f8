"""Golden outputs of scikit-learn's k-means and of the reference ``cluster_and_viz.py`` CLI.

Run from the repo root on a CPU machine (needs scikit-learn 1.7.2, pandas and tqdm, and /root/reference
for the CLI run; neither is read at test time):
    python tests/golden/make_golden_kmeans.py

Writes tests/golden/kmeans/:
* ``sklearn.npz``: for every ``kmeans_ref.CASES`` x ``kmeans_ref.SEEDS`` entry, on the float64 recipe
  input, ``<case>_seeds`` = ``kmeans_plusplus(X, k, random_state=seed)[1]`` and ``<case>_labels``,
  ``<case>_inertia``, ``<case>_n_iter`` of ``KMeans(k, n_init=n_init, random_state=seed).fit(X)``.
* ``cli/``: ``all_feature_clusters.tsv``, ``cluster_sizes.tsv``, ``clusters.txt`` (the concatenated
  ``clusters/cluster_<i>.tsv``, each after a ``== cluster_<i>.tsv`` line) and ``stdout.txt`` of the
  unmodified reference script (tests/golden/stubs_kmeans supplies matplotlib) on ``kmeans_ref.cli_reduced(334)``
  with ``kmeans_ref.CLI_FLAGS``; the test regenerates the input from the same function.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, GOLD)
sys.path.insert(0, os.path.dirname(GOLD))
import kmeans_ref  # noqa: E402
from make_golden_predict import REF  # noqa: E402

DST = os.path.join(GOLD, "kmeans")
STUBS = os.path.join(GOLD, "stubs_kmeans")
FEATURES_TSV = os.path.join(GOLD, "predict_sed", "deepsea_beluga_2002_features.tsv")


def sklearn_cases():
    from sklearn.cluster import KMeans, kmeans_plusplus
    out = {}
    for name, k, n_init in kmeans_ref.CASES:
        X = kmeans_ref.INPUTS[name]()
        for seed in kmeans_ref.SEEDS:
            case = kmeans_ref.case_name(name, k, n_init, seed)
            out[case + "_seeds"] = kmeans_plusplus(X, k, random_state=seed)[1].astype(np.int32)
            km = KMeans(k, n_init=n_init, random_state=seed).fit(X)
            out[case + "_labels"] = km.labels_.astype(np.int32)
            out[case + "_inertia"] = np.float64(km.inertia_)
            out[case + "_n_iter"] = np.int32(km.n_iter_)
    return out


def reference_cli():
    work = tempfile.mkdtemp(prefix="expecto_golden_kmeans_")
    os.makedirs(os.path.join(work, "in"))
    np.save(os.path.join(work, "in", "tf_idf_reduced_100.npy"), kmeans_ref.cli_reduced(kmeans_ref.CLI_MARKS))
    env = dict(os.environ, PYTHONPATH=STUBS + ":" + REF, OMP_NUM_THREADS="8")
    out = subprocess.run([sys.executable, os.path.join(REF, "cluster_and_viz.py"), "in", "--belugaFeatures",
                          FEATURES_TSV, *kmeans_ref.CLI_FLAGS, "-o", "out"], cwd=work, env=env, capture_output=True,
                         text=True)
    if out.returncode:
        sys.stderr.write(out.stderr)
        raise SystemExit(out.returncode)
    dst = os.path.join(DST, "cli")
    os.makedirs(dst, exist_ok=True)
    for name in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
        shutil.copy(os.path.join(work, "out", name), os.path.join(dst, name))
    with open(os.path.join(dst, "clusters.txt"), "w") as f:
        for i in range(30):
            f.write(f"== cluster_{i}.tsv\n")
            with open(os.path.join(work, "out", "clusters", f"cluster_{i}.tsv")) as src:
                f.write(src.read())
    with open(os.path.join(dst, "stdout.txt"), "w") as f:
        f.write(out.stdout)
    shutil.rmtree(work)


def main():
    os.makedirs(DST, exist_ok=True)
    np.savez_compressed(os.path.join(DST, "sklearn.npz"), **sklearn_cases())
    reference_cli()
    print("k-means golden outputs written to", DST)


if __name__ == "__main__":
    main()
