"""Time the model scores of ``expecto_amd.metrics`` at the size of a ``train_susztak`` batch: 256 models scored on
21,000 train rows and on 1,000 test rows (``rank2`` of the predictions and of the shared labels, then
``model_metrics``), and ``bootstrap_coef_stats`` of 800 bootstrap models with 20,020 coefficients (DESIGN.md
"Model metrics" records the figures).

    python tools/metrics_bench.py [--models 256] [--train-rows 21000] [--test-rows 1000] [--boot 800] \\
        [--coefs 20020] [--runs 5] [--cpu-models 8]

Prints one JSON line: medians over ``--runs`` of the device time (HIP events) of each step, and, when scipy and
sklearn are importable, the wall time of the reference's host loop (``pearsonr``, ``spearmanr``, ``r2_score`` per
model) over ``--cpu-models`` of the models, scaled up for the ratio, and of ``np.std`` / ``np.mean`` over the
bootstrap matrix.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(P, n, seed):
    rng = np.random.RandomState(seed)
    y = rng.standard_normal(n) * 2.0 + 1.0
    pred = (rng.uniform(0.2, 0.9, (P, 1)) * y + rng.standard_normal((P, n))).astype(np.float32)
    return pred, y


def cpu_loop(pred, y, models):
    try:
        from scipy.stats import pearsonr, spearmanr
        from sklearn.metrics import r2_score
    except ImportError:
        return None
    t0 = time.perf_counter()
    for m in range(models):
        pearsonr(y, pred[m])
        spearmanr(y, pred[m])
        r2_score(y_true=y, y_pred=pred[m])
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--train-rows", type=int, default=21000)
    ap.add_argument("--test-rows", type=int, default=1000)
    ap.add_argument("--boot", type=int, default=800)
    ap.add_argument("--coefs", type=int, default=20020)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cpu-models", type=int, default=8)
    a = ap.parse_args()
    import torch

    from expecto_amd import metrics
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU: a CPU run gives no time")
    out = {"models": a.models, "boot": a.boot, "coefs": a.coefs, "runs": a.runs}
    for tag, n in (("train", a.train_rows), ("test", a.test_rows)):
        pred, y = synth(a.models, n, seed=n)
        d_pred, d_y = torch.from_numpy(pred).cuda(), torch.from_numpy(y).cuda()
        metrics.model_metrics(d_pred, d_y)                       # warm-up: code objects, allocator
        torch.cuda.synchronize()
        t_rank, t_all = [], []
        for _ in range(a.runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            metrics.rank2(d_pred)
            metrics.rank2(d_y)
            ev[1].record()
            torch.cuda.synchronize()
            ev[2].record()
            metrics.model_metrics(d_pred, d_y)                   # ranks and scores, with the copy of [P, 3] back
            ev[3].record()
            torch.cuda.synchronize()
            t_rank.append(ev[0].elapsed_time(ev[1]))
            t_all.append(ev[2].elapsed_time(ev[3]))
        out.update({f"{tag}_rows": n, f"{tag}_rank2_ms": round(float(np.median(t_rank)), 3),
                    f"{tag}_model_metrics_ms": round(float(np.median(t_all)), 3),
                    f"{tag}_model_metrics_ms_all": [round(t, 3) for t in t_all]})
        k = min(a.cpu_models, a.models)
        cpu = cpu_loop(pred, y, k) if k > 0 else None
        if cpu is not None:
            out.update({f"{tag}_cpu_ms": round(cpu, 3), f"{tag}_cpu_models": k,
                        f"{tag}_ratio_cpu_scaled_over_gpu": round(cpu * a.models / k / out[f"{tag}_model_metrics_ms"], 1)})
    rng = np.random.RandomState(7)
    W = rng.standard_normal((a.boot, a.coefs)) * 0.01
    w_main = rng.standard_normal(a.coefs) * 0.01
    d_W, d_w = torch.from_numpy(W).cuda(), torch.from_numpy(w_main).cuda()
    metrics.bootstrap_coef_stats(d_W, d_w)
    torch.cuda.synchronize()
    t_cs = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        metrics.bootstrap_coef_stats(d_W, d_w)
        e1.record()
        torch.cuda.synchronize()
        t_cs.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    se = np.std(W, axis=0, ddof=1)
    _ = w_main / se, se / np.abs(np.mean(W, axis=0))
    out.update(coef_stats_ms=round(float(np.median(t_cs)), 3), coef_stats_ms_all=[round(t, 3) for t in t_cs],
               coef_stats_numpy_ms=round(1e3 * (time.perf_counter() - t0), 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
