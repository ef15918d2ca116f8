"""Throughput of gblinear training (expecto_gblinear_train_round) at the ExPecto shape.

    python tools/train_bench.py [--out profiles/train_bench.json] [--rounds 10] [--repeats 3]

Shape: n = 22,000 genes x F = 20,020 features, batches of B = 1, 64, 256, 1024 models sharing one
column-major float32 matrix (1.76 GB).  Each measurement is `rounds` launches of the round kernel
between two device events after two warm-up rounds; the batch sizes are run in turn, `repeats`
times over, and the median and the spread of each are reported:

* ms per round, models x rounds per second;
* achieved bytes/s counting 2 * n * F * 4 bytes per model-round (the predict pass and the
  coordinate pass each read X once) against the 8 TB/s HBM peak.  A batch shares the columns
  through the L2s and the infinity cache, so this figure may exceed the HBM rate: it counts the
  bytes the models consume, not the bytes the memory delivers;
* the B = 1 fetch probe: the same launch with n = 1,024 rows.  The kernel runs the same
  instructions for every n (24 row slots per lane, range-checked loads), so this run differs only
  in fetching 1/21 of the bytes: equal time per feature means the chain reduction -> dw -> update
  bounds a single model, not the column fetch;
* the same algorithm in torch on the CPU (16 threads), one round, as the baseline.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from expecto_amd import _lib  # noqa: E402
from expecto_amd.xgblinear import ColMatrix  # noqa: E402

HBM_PEAK = 8.0e12
HYPER = dict(eta=0.01, lam=100.0, alpha=0.0, lam_bias=0.0, base=2.0)


def gpu_rounds(lib, Xc, n, y, B, rounds):
    """ms per round of `rounds` launches for B models (fresh weights, 2 warm-up rounds)."""
    dev = Xc.device
    w = torch.zeros(B, Xc.F + 1, device=dev)
    sh = torch.empty(B, Xc.F, dtype=torch.float64, device=dev)

    def launch(first):
        _lib.check(lib.expecto_gblinear_train_round(
            _lib.dptr(Xc.data), Xc.ld, n, Xc.F, B, _lib.dptr(y), y.shape[1], None, 0, _lib.dptr(w), _lib.dptr(sh),
            int(first), HYPER["eta"], HYPER["lam"], HYPER["alpha"], HYPER["lam_bias"], HYPER["base"], None,
            _lib.stream_ptr()), "train_round")

    launch(True)
    launch(False)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(rounds):
        launch(False)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / rounds


def cpu_round(Xt, y):
    """One round of the same steps in torch on the CPU: Xt [F, n] float32, y [B, n]; seconds."""
    B, n = y.shape
    F = Xt.shape[0]
    w = torch.zeros(B, F)
    b = torch.zeros(B)
    t0 = time.perf_counter()
    p = (b + HYPER["base"])[:, None].repeat(1, n)
    for j in range(F):
        p = p + Xt[j][None, :] * w[:, j:j + 1]
    g = p - y
    db = (HYPER["eta"] * (-g.double().sum(1) / n)).float()
    g = g + db[:, None]
    for j in range(F):
        x = Xt[j][None, :]
        sg = (g * x).double().sum(1)
        shj = (x * x).double().sum(1)
        wj = w[:, j].double()
        d = torch.where(shj < 1e-5, torch.zeros_like(sg), -(sg + HYPER["lam"] * wj) / (shj + HYPER["lam"]))
        dw = (HYPER["eta"] * d).float()
        w[:, j] += dw
        g = g + x * dw[:, None]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/train_bench.json")
    ap.add_argument("--n", type=int, default=22000)
    ap.add_argument("--features", type=int, default=20020)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 256, 1024])
    ap.add_argument("--cpu-batches", type=int, nargs="*", default=[1, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("train_bench needs a GPU: a CPU run says nothing about it")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n, F = a.n, a.features
    g = torch.Generator(device=dev).manual_seed(0)
    Xc = ColMatrix(torch.zeros(0, F), device=dev)          # filled in place: no [n, F] copy on the way
    Xc.n, Xc.ld = n, (n + 63) // 64 * 64
    Xc.data = torch.zeros(F, Xc.ld, device=dev)
    Xc.data[:, :n] = torch.randn(F, n, device=dev, generator=g) * (0.01 + 2.99 * torch.rand(F, 1, device=dev, generator=g))
    Bmax = max(a.batches)
    y = 2.0 + torch.randn(Bmax, n, device=dev, generator=g)
    bytes_per_model_round = 2.0 * n * F * 4

    ms = {B: [] for B in a.batches}
    probe = []
    for _ in range(a.repeats):                               # alternate the sizes, repeat the lot
        for B in a.batches:
            ms[B].append(gpu_rounds(lib, Xc, n, y[:B], B, a.rounds))
        probe.append(gpu_rounds(lib, Xc, 1024, y[:1, :1024].contiguous(), 1, a.rounds))
    res = {"shape": {"n": n, "F": F, "rounds": a.rounds, "repeats": a.repeats}, "device": torch.cuda.get_device_name(0),
           "bytes_per_model_round": bytes_per_model_round, "gpu": [], "cpu_torch_16_threads": []}
    for B in a.batches:
        med = statistics.median(ms[B])
        res["gpu"].append({"B": B, "ms_per_round": med, "ms_min": min(ms[B]), "ms_max": max(ms[B]),
                           "model_rounds_per_s": B / med * 1e3, "us_per_feature_step": med * 1e3 / F,
                           "consumed_bytes_per_s": B * bytes_per_model_round / med * 1e3,
                           "share_of_hbm_peak": B * bytes_per_model_round / med * 1e3 / HBM_PEAK})
    pm = statistics.median(probe)
    res["b1_fetch_probe"] = {"n": 1024, "ms_per_round": pm, "ms_min": min(probe), "ms_max": max(probe),
                             "us_per_feature_step": pm * 1e3 / F}
    torch.set_num_threads(16)
    Xt = Xc.data[:, :n].cpu().contiguous()
    for B in a.cpu_batches:
        s = cpu_round(Xt, y[:B].cpu())
        res["cpu_torch_16_threads"].append({"B": B, "s_per_round": s, "model_rounds_per_s": B / s})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
