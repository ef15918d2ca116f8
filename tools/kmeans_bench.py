"""Times of the batched k-means at the reference's shape (DESIGN.md "k-means of the SVD coordinates").

    python tools/kmeans_bench.py                  # device: (a) the elbow sweep, (b) k = 197 alone, (c) k = 30 alone
    python tools/kmeans_bench.py --baseline       # CPU: (d) sklearn's loop over the same sweep

The matrix is synthetic float32 [2002, 20] (structureless Gaussian: the longest Lloyd runs), converted
to float64.  (a) is the reference's commented-out sweep, ``k in range(2, 200, 5)`` with ``n_init = 1``,
as one ``kmeans_sweep``: 40 problems in one seeding call and one Lloyd call.  The two calls are timed
apart with events inside ``run_problems`` (uploads before the first event, downloads after the last),
after one warm-up run, ``--reps`` times; the wall time of the whole ``kmeans_sweep`` (draws, uploads,
both calls, downloads) is printed beside them.  The batch overlaps its problems if (a) is well under
40 x (b).  Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, D = 2002, 20
SWEEP = list(range(2, 200, 5))


def matrix():
    return np.random.RandomState(102).normal(size=(N, D)).astype(np.float32).astype(np.float64)


def device(reps):
    import torch

    from expecto_amd import cluster_and_viz
    X = matrix()
    for what, ks in (("(a) sweep range(2, 200, 5)", SWEEP), ("(b) k = 197 alone", [197]), ("(c) k = 30 alone", [30])):
        cluster_and_viz.kmeans_sweep(X, ks, seed=0)          # warm-up
        torch.cuda.synchronize()
        seeding, lloyd, wall = [], [], []
        for _ in range(reps):
            t = {}
            t0 = time.perf_counter()
            res = cluster_and_viz.kmeans_sweep(X, ks, seed=0, timings=t)
            wall.append((time.perf_counter() - t0) * 1e3)
            seeding.append(t["seeding_ms"])
            lloyd.append(t["lloyd_ms"])
        print(json.dumps({"what": what, "n": N, "d": D, "problems": len(ks), "seeding_ms": seeding, "lloyd_ms": lloyd,
                          "wall_ms": wall, "best_seeding_ms": min(seeding), "best_lloyd_ms": min(lloyd),
                          "best_device_ms": min(s + l for s, l in zip(seeding, lloyd)),
                          "n_iter": [r.n_iter for r in res], "inertia_last": res[-1].inertia}), flush=True)


def baseline():
    from sklearn.cluster import KMeans
    X = matrix()
    for dtype in (np.float64, np.float32):
        Xd = X.astype(dtype)
        KMeans(n_clusters=2, random_state=0).fit(Xd)
        t0 = time.perf_counter()
        iters = [int(KMeans(n_clusters=k, random_state=0).fit(Xd).n_iter_) for k in SWEEP]
        t1 = time.perf_counter()
        print(json.dumps({"what": "(d) sklearn KMeans(n_clusters=k, random_state=0).fit, one call per k", "dtype":
                          np.dtype(dtype).name, "n": N, "d": D, "problems": len(SWEEP), "total_ms": (t1 - t0) * 1e3,
                          "n_iter": iters, "cpus": os.cpu_count(),
                          "threads": os.environ.get("OMP_NUM_THREADS", "unset")}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--baseline", action="store_true")
    a = p.parse_args()
    baseline() if a.baseline else device(a.reps)


if __name__ == "__main__":
    main()
