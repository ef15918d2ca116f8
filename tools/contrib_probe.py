"""Time of the fused attribution (expecto_variant_contrib) against the route available without it.

    python tools/contrib_probe.py [--out profiles/contrib_probe.json] [--iters 50] [--repeats 5]

Shape: n = 4,096 variants, 9 shifts, all 2,002 marks, 10 clusters, for 1 and 16 models.

* fused: one ``variant_contributions`` call (contrib, total, prop, clu, clu_prop).
* torch: two ``variant_reduce`` calls into float64 ``[n, 20020]`` features, then the attribution
  in torch float64 device ops in the same process (difference, einsum over the 10 decay rows,
  sums, divisions, a ``[nk, n_clu]`` membership matmul).

Each measurement is ``iters`` calls between two device events after one warm-up call; the two
routes and the two model counts alternate, ``repeats`` times over, and the median and the spread
are reported.  Bytes are the ones the fused algorithm needs: the effects read once
(2 * 9 * n * 2002 * 4), the weights once, every output written once; their rate is given as a share
of the 8 TB/s HBM peak.  The torch route moves at least 4 * n * 20020 * 8 more (the features
written and read back).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from expecto_amd.features import variant_contributions, variant_reduce, variant_tables  # noqa: E402

HBM_PEAK = 8.0e12
SHIFTS = [0, -200, -400, -600, -800, 200, 400, 600, 800]


def timed(fn, iters):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/contrib_probe.json")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("contrib_probe needs a GPU: a CPU run says nothing about it")
    dev = torch.device("cuda", 0)
    n, F, S, n_clu = a.n, 2002, len(SHIFTS), 10
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.randn(S, n, F, device=dev, generator=g) * 0.05
    alt = ref + torch.randn(S, n, F, device=dev, generator=g) * 0.01
    rng = np.random.default_rng(0)
    dist = rng.integers(-20000, 20000, n)
    strand_plus = rng.random(n) < 0.5
    keep = np.arange(F)
    label = rng.integers(0, n_clu, F)
    clusters = [np.nonzero(label == c)[0].tolist() for c in range(n_clu)]
    onehot = torch.zeros(F, n_clu, dtype=torch.float64, device=dev)
    onehot[torch.arange(F, device=dev), torch.from_numpy(label).to(dev)] = 1.0
    tables = variant_tables(dist, strand_plus, SHIFTS, dev)
    weights = {M: rng.normal(0.01, 0.02, (M, 10 * F)) for M in a.models}
    w_dev = {M: torch.from_numpy(weights[M]).to(dev).view(M, 10, F) for M in a.models}

    def fused(M):
        return variant_contributions(ref, alt, dist, strand_plus, SHIFTS, keep, weights[M], clusters)

    def torch_route(M):
        fr, fa = variant_reduce(ref, tables), variant_reduce(alt, tables)
        D = (fa - fr).view(n, 10, F)
        contrib = torch.einsum("mkf,nkf->mnf", w_dev[M], D)
        total = contrib.sum(-1)
        clu = contrib @ onehot
        return contrib, total, contrib / total[..., None], clu, clu / clu.sum(-1, keepdim=True)

    # the two routes agree (another summation order: last bits only)
    x, y = fused(a.models[0]), torch_route(a.models[0])
    err = float(((x.contrib - y[0]).abs().max() / y[0].abs().max()).cpu())
    if not err < 1e-12:
        raise AssertionError(f"fused and torch contributions differ: {err}")
    del x, y

    ms = {(route, M): [] for route in ("fused", "torch") for M in a.models}
    for _ in range(a.repeats):
        for M in a.models:
            ms["fused", M].append(timed(lambda: fused(M), a.iters))
            ms["torch", M].append(timed(lambda: torch_route(M), a.iters))
    res = {"shape": {"n": n, "n_shift": S, "marks": F, "clusters": n_clu, "iters": a.iters, "repeats": a.repeats},
           "device": torch.cuda.get_device_name(0), "max_rel_diff_contrib": err, "runs": []}
    for M in a.models:
        need = 2 * S * n * F * 4 + M * 10 * F * 8 + M * n * (2 * F + 1 + 2 * n_clu) * 8
        row = {"models": M, "fused_bytes": need}
        for route in ("fused", "torch"):
            t = ms[route, M]
            row[route] = {"ms": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        row["fused"]["bytes_per_s"] = need / row["fused"]["ms"] * 1e3
        row["fused"]["share_of_hbm_peak"] = row["fused"]["bytes_per_s"] / HBM_PEAK
        row["torch_over_fused"] = row["torch"]["ms"] / row["fused"]["ms"]
        res["runs"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
