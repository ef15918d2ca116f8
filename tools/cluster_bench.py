"""Times of the Ward clustering at the two real shapes (DESIGN.md "Ward clustering of the marks").

    python tools/cluster_bench.py                     # device: kernel alone, then ward_tree's stages
    python tools/cluster_bench.py --baseline          # CPU: scipy pdist + ward (what sklearn runs)

Shapes: grouped (2002 marks x 18000 genes x 10) and ungrouped (20020 features x 18000 genes), on
synthetic non-negative data.  The kernel is timed with events after a warm-up call; the stages of
``ward_tree`` (kernel, copy of the condensed matrix to the host, host linkage) with the wall clock.
Kernel efficiency counts 3 flops per pair and dimension (subtract, multiply, add) against the fp64
vector peak, 78.6 TFLOP/s (256 CUs x 4 SIMDs x 32 flop/clk x 2.4 GHz, FMA counted as two); without
FMA, which the fixed rounding forbids, a VALU instruction is one flop and the ceiling is half of that.
The baseline runs the ungrouped shape at ``--baseline_n`` points and scales by n^2 d: an extrapolation.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"grouped": (2002, 180000), "ungrouped": (20020, 18000)}
FP64_VECTOR_PEAK = 256 * 4 * 32 * 2.4e9


def device(shapes, reps):
    import torch

    from expecto_amd import _lib, interpret_features

    lib = _lib.load()
    for name in shapes:
        n, d = SHAPES[name]
        x = torch.rand(n, d, dtype=torch.float64, device="cuda")
        cond = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device="cuda")
        call = lambda: _lib.check(lib.expecto_pairwise_euclidean(_lib.dptr(x), n, d, d, _lib.dptr(cond),
                                                                 _lib.stream_ptr()), "expecto_pairwise_euclidean")
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
        best = min(ms)
        flops = 3.0 * (n * (n - 1) // 2) * d
        print(json.dumps({"what": "kernel", "shape": name, "n": n, "d": d, "ms": ms, "best_ms": best,
                          "tflops": flops / best / 1e9, "fraction_of_fp64_vector_peak": flops / (best * 1e-3) / FP64_VECTOR_PEAK}),
              flush=True)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = cond.cpu().numpy()
        t2 = time.perf_counter()
        interpret_features._link(host, n)
        t3 = time.perf_counter()
        print(json.dumps({"what": "ward_tree stages", "shape": name, "kernel_s": t1 - t0, "d2h_s": t2 - t1,
                          "linkage_s": t3 - t2, "total_s": t3 - t0}), flush=True)
        del x, cond, host


def baseline(shapes, baseline_n):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist

    for name in shapes:
        n_full, d = SHAPES[name]
        n = n_full if name == "grouped" else min(baseline_n, n_full)
        x = np.random.default_rng(0).random((n, d))
        t0 = time.perf_counter()
        cond = pdist(x)
        t1 = time.perf_counter()
        linkage(cond, "ward")
        t2 = time.perf_counter()
        scale = (n_full / n) ** 2
        print(json.dumps({"what": "scipy baseline", "shape": name, "n_run": n, "d": d, "pdist_s": t1 - t0,
                          "ward_s": t2 - t1, "extrapolated": n != n_full, "pdist_s_at_full_n": (t1 - t0) * scale,
                          "ward_s_at_full_n": (t2 - t1) * scale, "cpus": os.cpu_count()}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--shape", choices=["grouped", "ungrouped", "both"], default="both")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--baseline", action="store_true")
    p.add_argument("--baseline_n", type=int, default=2002)
    a = p.parse_args()
    shapes = list(SHAPES) if a.shape == "both" else [a.shape]
    baseline(shapes, a.baseline_n) if a.baseline else device(shapes, a.reps)


if __name__ == "__main__":
    main()
