"""Times of the exact t-SNE at the reference's shape (DESIGN.md "t-SNE of the SVD coordinates").

    python tools/tsne_bench.py                  # device: the affinity call and the descent's calls
    python tools/tsne_bench.py --baseline       # CPU: sklearn's TSNE(method='exact') on the same matrix

The matrix is synthetic [2002, 20]: 30 integer centres with integer scatter around them.  The device
run is ``cluster_and_viz.tsne(X, max_iter=1000)`` with its defaults (perplexity 30, PCA start), timed
with events around the affinity call and around each of the descent's calls (one per 50 iterations;
the host reads three numbers in between), after one short warm-up run, ``--reps`` times; the wall time
of the whole call (SVD for the start, uploads, calls, downloads) is printed beside them.  Prints one
JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, D, ITERATIONS = 2002, 20, 1000


def matrix():
    rng = np.random.RandomState(11)
    centres = rng.randint(-12, 13, size=(30, D))
    return (centres[rng.randint(0, 30, size=N)] + rng.randint(-5, 6, size=(N, D))).astype(np.float64)


def device(reps):
    from expecto_amd import cluster_and_viz
    X = matrix()
    cluster_and_viz.tsne(X, max_iter=50)          # warm-up
    for _ in range(reps):
        t = {}
        t0 = time.perf_counter()
        res = cluster_and_viz.tsne(X, max_iter=ITERATIONS, timings=t)
        wall = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"what": "tsne(X, max_iter=1000)", "n": N, "d": D, "affinities_ms": t["affinities_ms"],
                          "descent_ms": t["descent_ms"], "wall_ms": wall, "n_iter": res.n_iter,
                          "kl_divergence": res.kl_divergence}), flush=True)


def baseline():
    from sklearn.manifold import TSNE
    X = matrix()
    t0 = time.perf_counter()
    ts = TSNE(n_components=2, method="exact", init="pca", random_state=0, max_iter=ITERATIONS)
    ts.fit_transform(X)
    print(json.dumps({"what": "sklearn TSNE(method='exact', init='pca', max_iter=1000).fit_transform", "n": N, "d": D,
                      "total_ms": (time.perf_counter() - t0) * 1e3, "n_iter": int(ts.n_iter_) + 1,
                      "kl_divergence": float(ts.kl_divergence_), "cpus": os.cpu_count(),
                      "threads": os.environ.get("OMP_NUM_THREADS", "unset")}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--baseline", action="store_true")
    a = p.parse_args()
    baseline() if a.baseline else device(a.reps)


if __name__ == "__main__":
    main()
