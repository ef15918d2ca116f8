"""Times of the silhouette sweep at the two real shapes (DESIGN.md "Silhouette sweep").

    python tools/silhouette_bench.py                  # device: the kernels alone, then silhouette_sweep's stages
    python tools/silhouette_bench.py --baseline       # CPU: sklearn's silhouette_samples(metric='precomputed')

Shapes: grouped (2,002 points) and ungrouped (20,020 points), k = 2..499, on synthetic points of 16
dimensions (the sweep reads distances only; the tree is this program's own Ward tree of them).  Each
kernel is timed with events after a warm-up call, best of ``--reps``; the node sums in both layouts
of the distances (square, after the expansion kernel, and condensed).  Bytes are what the algorithm
needs from shapes: node sums read one distance per (member, point) and write S; the cuts read one sum
per (cut, active node, point) and write the samples.  Most of those reads hit the caches, so the
share of the 8 TB/s HBM peak is a rate of useful bytes, not of HBM traffic.  The stages of
``silhouette_sweep`` (host plan, uploads + kernels + download, host means) use the wall clock.  The
baseline runs sklearn on the grouped shape only, one call per k.  Prints one JSON line per
measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"grouped": 2002, "ungrouped": 20020}
K_MIN, K_MAX, DIMS = 2, 499, 16
HBM_PEAK = 8e12


def timed(call, reps):
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def device(shapes, reps):
    import torch

    from expecto_amd import _lib, interpret_features

    lib = _lib.load()
    ks = list(range(K_MIN, K_MAX + 1))
    for name in shapes:
        n = SHAPES[name]
        x = torch.from_numpy(np.random.default_rng(n).gamma(0.7, 2.0, (n, DIMS))).cuda()
        t0 = time.perf_counter()
        children, _, cond = interpret_features.ward_tree(x, return_condensed=True)
        t1 = time.perf_counter()
        plan = interpret_features.plan_sweep(children, n, ks)
        t2 = time.perf_counter()
        n_nodes, n_cuts = len(plan.sizes), len(ks)
        d = {k: torch.from_numpy(getattr(plan, k)).cuda() for k in ("node_ptr", "members", "sizes", "cut_ptr", "active", "own")}
        sq = torch.empty((n, n), dtype=torch.float64, device="cuda")
        S = torch.empty((n_nodes, n), dtype=torch.float64, device="cuda")
        samples = torch.empty((n_cuts, n), dtype=torch.float64, device="cuda")
        st = _lib.stream_ptr
        expand = lambda: _lib.check(lib.expecto_square_distances(_lib.dptr(cond), n, _lib.dptr(sq), st()), "square")
        sums = lambda dist, square: _lib.check(lib.expecto_silhouette_node_sums(
            _lib.dptr(dist), square, n, plan.node_ptr.ctypes.data, _lib.dptr(d["node_ptr"]), _lib.dptr(d["members"]), n_nodes,
            _lib.dptr(S), st()), "node sums")
        cuts = lambda: _lib.check(lib.expecto_silhouette_cuts(
            _lib.dptr(S), n, n_nodes, _lib.dptr(d["sizes"]), plan.cut_ptr.ctypes.data, _lib.dptr(d["cut_ptr"]),
            _lib.dptr(d["active"]), _lib.dptr(d["own"]), n_cuts, _lib.dptr(samples), st()), "cuts")
        sum_bytes = 8 * (len(plan.members) + n_nodes) * n
        cut_bytes = 8 * (len(plan.active) + n_cuts) * n + 4 * n_cuts * n
        work = (("square_distances", expand, 8 * (n * (n - 1) // 2 + n * n)),
                ("node_sums square", lambda: sums(sq, 1), sum_bytes), ("node_sums condensed", lambda: sums(cond, 0), sum_bytes),
                ("cuts", cuts, cut_bytes))
        for what, call, nbytes in work:
            ms = timed(call, reps)
            best = min(ms)
            print(json.dumps({"what": what, "shape": name, "n": n, "k": [K_MIN, K_MAX], "nodes": n_nodes,
                              "members": len(plan.members), "ms": ms, "best_ms": best, "bytes": nbytes,
                              "tb_per_s": nbytes / best / 1e9, "share_of_8_tb_per_s": nbytes / (best * 1e-3) / HBM_PEAK}),
                  flush=True)
        del sq, S, samples
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        scores, _ = interpret_features.silhouette_sweep(children, cond, n, ks)
        t4 = time.perf_counter()
        print(json.dumps({"what": "silhouette_sweep stages", "shape": name, "ward_tree_s": t1 - t0, "plan_s": t2 - t1,
                          "sweep_total_s": t4 - t3, "workspace_bytes": 8 * n_nodes * n, "samples_bytes": 8 * n_cuts * n,
                          "square_bytes": 8 * n * n, "best_k": int(np.argmax(scores)) + K_MIN}), flush=True)
        del cond, d


def baseline():
    from scipy.cluster.hierarchy import ward
    from scipy.spatial.distance import pdist, squareform
    from sklearn.metrics import silhouette_samples

    from expecto_amd.interpret_features import cut_tree

    n = SHAPES["grouped"]
    cond = pdist(np.random.default_rng(n).gamma(0.7, 2.0, (n, DIMS)))
    children = ward(cond)[:, :2].astype(np.int64)
    D = squareform(cond)
    t0 = time.perf_counter()
    for k in range(K_MIN, K_MAX + 1):
        silhouette_samples(D, cut_tree(children, n, k), metric="precomputed")
    t1 = time.perf_counter()
    print(json.dumps({"what": "sklearn silhouette_samples(metric='precomputed'), one call per k", "shape": "grouped", "n": n,
                      "k": [K_MIN, K_MAX], "total_s": t1 - t0, "cpus": os.cpu_count()}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--shape", choices=["grouped", "ungrouped", "both"], default="both")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--baseline", action="store_true")
    a = p.parse_args()
    baseline() if a.baseline else device(list(SHAPES) if a.shape == "both" else [a.shape], a.reps)


if __name__ == "__main__":
    main()
