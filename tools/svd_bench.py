"""Times of the tf-idf SVD kernels at the real mark count (DESIGN.md "SVD of the mark tracks").

    python tools/svd_bench.py                 # device kernels with events, host eigh with the wall clock
    python tools/svd_bench.py --baseline      # CPU: sklearn TruncatedSVD(100).fit on the same shape

Shape: m = 2002 marks, n = 204,800 columns (1,024 genes x 200), k = 100, synthetic data made on the
device; no files are read.  ``--columns 51200`` is one chunk of a fit with the default gene batch of
256.  Each kernel is timed with events after a warm-up call.  The baseline's matrix comes from the
tests' restatement (tests/svd_ref.tfidf); only sklearn's fit is timed.  The Gram
kernel's rate counts the flops it executes, 2 x 64 x 64 x n per upper-triangle tile (528 tiles: 0.54
of the full 2 m^2 n), against the fp64 matrix peak of 78.6 TFLOP/s.  Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12


def timed(torch, call, reps):
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


def device(m, n, k, reps):
    import torch

    from expecto_amd import _lib

    lib = _lib.load()
    s = _lib.stream_ptr()
    D = torch.rand(n, m, dtype=torch.float32, device="cuda")
    keep = torch.arange(m, dtype=torch.int32, device="cuda")
    idf = torch.empty(n, dtype=torch.float64, device="cuda")
    rowsum = torch.zeros(m, dtype=torch.float64, device="cuda")
    H = torch.zeros(m, m, dtype=torch.float64, device="cuda")
    P = torch.randn(k, m, dtype=torch.float64, device="cuda")
    comps = torch.empty(k, n, dtype=torch.float32, device="cuda")
    X = torch.zeros(m, k, dtype=torch.float64, device="cuda")
    gb, tb = lib.expecto_tfidf_gram_workspace(m, n), lib.expecto_tfidf_transform_workspace(m, k, n)
    ws = torch.empty(max(gb, tb) // 8, dtype=torch.float64, device="cuda")
    common = (D.data_ptr(), n, m, keep.data_ptr(), m)
    calls = {
        "stats": lambda: _lib.check(lib.expecto_tfidf_stats(*common, idf.data_ptr(), rowsum.data_ptr(), s), "stats"),
        "gram": lambda: _lib.check(lib.expecto_tfidf_gram(*common, idf.data_ptr(), H.data_ptr(), ws.data_ptr(), gb, s),
                                   "gram"),
        "project": lambda: _lib.check(lib.expecto_tfidf_project(*common, idf.data_ptr(), P.data_ptr(), k,
                                                                comps.data_ptr(), n, s), "project"),
        "transform": lambda: _lib.check(lib.expecto_tfidf_transform(*common, idf.data_ptr(), comps.data_ptr(), n, k,
                                                                    X.data_ptr(), ws.data_ptr(), tb, s), "transform"),
    }
    tiles = ((m + 63) // 64) * ((m + 63) // 64 + 1) // 2
    for name, call in calls.items():
        ms = timed(torch, call, reps)
        rec = {"what": name, "m": m, "n": n, "k": k, "ms": ms, "best_ms": min(ms)}
        if name == "gram":
            flops = 2.0 * 64 * 64 * n * tiles
            rec.update(parts=lib.expecto_tfidf_gram_parts(m, n), executed_tflops=flops / min(ms) / 1e9,
                       fraction_of_fp64_matrix_peak=flops / (min(ms) * 1e-3) / FP64_MATRIX_PEAK,
                       full_matrix_equivalent_tflops=2.0 * m * m * n / min(ms) / 1e9)
        elif name in ("project", "transform"):
            rec.update(tflops=2.0 * m * k * n / min(ms) / 1e9)
        print(json.dumps(rec), flush=True)
    G = (H / H.diagonal().max()).cpu().numpy()
    t0 = time.perf_counter()
    np.linalg.eigh(G)
    print(json.dumps({"what": "host eigh", "m": m, "s": time.perf_counter() - t0,
                      "threads": os.environ.get("OMP_NUM_THREADS")}), flush=True)


def baseline(m, n, k):
    from sklearn.decomposition import TruncatedSVD

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import svd_ref      # the tests' restatement builds the tf-idf matrix; only the fit is timed

    X = np.random.default_rng(0).random((n, m), dtype=np.float32)
    A = svd_ref.tfidf(X, np.arange(m)).astype(np.float32)      # [m, n], the dtype the reference fits
    del X
    t0 = time.perf_counter()
    TruncatedSVD(n_components=k).fit(A)
    t1 = time.perf_counter()
    print(json.dumps({"what": "sklearn baseline", "m": m, "n": n, "k": k, "fit_s": t1 - t0,
                      "threads": os.environ.get("OMP_NUM_THREADS")}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--marks", type=int, default=2002)
    p.add_argument("--columns", type=int, default=204800)
    p.add_argument("--components", type=int, default=100)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--baseline", action="store_true")
    a = p.parse_args()
    baseline(a.marks, a.columns, a.components) if a.baseline else device(a.marks, a.columns, a.components, a.reps)


if __name__ == "__main__":
    main()
