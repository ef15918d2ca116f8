"""What cross-validated gblinear training costs at the ExPecto shape (n = 22,000 x F = 20,020).

    python tools/train_cv_bench.py [--parent-lib PATH] [--out profiles/train_cv_bench.jsonl]

Device events around `rounds` launches after two warm-up rounds, the configurations run in turn and
the lot repeated `repeats` times; every figure is a median with its min and max.  One JSON line
per measurement:

1. ``round_b256``: ms per round of 256 models through the per-model table
   (expecto_gblinear_train_round_hp), through this build's scalar entry point, and -- with
   ``--parent-lib``, a libexpecto_hip.so built from the commit before the table existed -- through
   that build's scalar entry point.  The three run the same arithmetic; a difference beyond the
   spread the tool reports is a finding.
2. ``cv_160``: one ``xgblinear.cv`` call with T = 1, an 8 x 4 grid and K = 5 (160 models), 10 rounds,
   wall clock with a device synchronise at both ends, against 160 sequential B = 1 fits by the
   scalar entry point (of the parent library when given), each with the launches ``train`` makes:
   the rounds, an rmse per round, one predict_cols at the end.
3. ``cv_rmse_share``: the 160-model round loop of ``cv`` with events around the round launch and
   around the two rmse launches (train and held-out weights) that follow it.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from expecto_amd import _lib, xgblinear  # noqa: E402
from expecto_amd.xgblinear import ColMatrix  # noqa: E402

HYPER = (0.01, 100.0, 0.0, 0.0)
BASE = 2.0


def load_parent(path):
    """The four training entry points of another build of the library (local symbols)."""
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name in ("expecto_gblinear_train_round", "expecto_gblinear_predict_cols", "expecto_gblinear_rmse"):
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "spread": (max(ms) - min(ms)) / statistics.median(ms)}


def rounds_ms(launch, rounds):
    launch(True)
    launch(False)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(rounds):
        launch(False)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / rounds


def round_launcher(lib, Xc, y, h, B, hyper_dev=None):
    """launch(first) for B models on fresh weights: the scalar entry point of `lib`, or the table."""
    w = torch.zeros(B, Xc.F + 1, device=Xc.device)
    sh = torch.empty(B, Xc.F, dtype=torch.float64, device=Xc.device)
    head = (_lib.dptr(Xc.data), Xc.ld, Xc.n, Xc.F, B, _lib.dptr(y), y.shape[1] if y.shape[0] > 1 else 0,
            _lib.dptr(h) if h is not None else None, Xc.n if h is not None else 0, _lib.dptr(w), _lib.dptr(sh))

    def launch(first, pred=None):
        tail = (BASE, _lib.dptr(pred) if pred is not None else None, _lib.stream_ptr())
        if hyper_dev is None:
            st = lib.expecto_gblinear_train_round(*head, int(first), *HYPER, *tail)
        else:
            st = lib.expecto_gblinear_train_round_hp(*head, int(first), _lib.dptr(hyper_dev), *tail)
        assert st == 0, st

    launch.w = w
    return launch


def sequential_fits(lib, Xc, y, folds_h, n_fits, rounds):
    """n_fits B = 1 fits one after the other with the launches of ``train``; wall-clock seconds."""
    n, dev = Xc.n, Xc.device
    pred = torch.empty(1, n, device=dev)
    out = torch.zeros(rounds, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_fits):
        h = folds_h[i % len(folds_h)]
        launch = round_launcher(lib, Xc, y, h, 1)

        def rmse(r):
            assert lib.expecto_gblinear_rmse(_lib.dptr(pred), _lib.dptr(y), 0, _lib.dptr(h), 0, n, 1,
                                             _lib.dptr(out[r:]), _lib.stream_ptr()) == 0

        for r in range(rounds):
            launch(r == 0, pred if r else None)
            if r:
                rmse(r - 1)
        assert lib.expecto_gblinear_predict_cols(_lib.dptr(Xc.data), Xc.ld, n, Xc.F, 1, _lib.dptr(launch.w), BASE,
                                                 _lib.dptr(pred), _lib.stream_ptr()) == 0
        rmse(rounds - 1)
        out.cpu()                                   # the history comes back to the host, as in train
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/train_cv_bench.jsonl")
    ap.add_argument("--parent-lib", default=None, help="libexpecto_hip.so of the parent commit")
    ap.add_argument("--n", type=int, default=22000)
    ap.add_argument("--features", type=int, default=20020)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seq-fits", type=int, default=160, help="sequential B = 1 fits to time (160: the whole grid)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("train_cv_bench needs a GPU: a CPU run says nothing about it")
    lib = _lib.load()
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    dev = torch.device("cuda", 0)
    n, F = a.n, a.features
    g = torch.Generator(device=dev).manual_seed(0)
    Xc = ColMatrix(torch.zeros(0, F), device=dev)          # filled in place: no [n, F] copy on the way
    Xc.n, Xc.ld = n, (n + 63) // 64 * 64
    Xc.data = torch.zeros(F, Xc.ld, device=dev)
    Xc.data[:, :n] = torch.randn(F, n, device=dev, generator=g) * (0.01 + 2.99 * torch.rand(F, 1, device=dev, generator=g))
    y = 2.0 + torch.randn(256, n, device=dev, generator=g)
    meta = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "n": n, "F": F,
            "rounds": a.rounds, "repeats": a.repeats}
    lines = []

    # 1. the three round kernels at B = 256
    table = torch.tensor([HYPER] * 256, dtype=torch.float64, device=dev)
    configs = {"hp": round_launcher(lib, Xc, y, None, 256, table), "scalar": round_launcher(lib, Xc, y, None, 256)}
    if parent is not None:
        configs["parent_scalar"] = round_launcher(parent, Xc, y, None, 256)
    ms = {k: [] for k in configs}
    for _ in range(a.repeats):
        for k, launch in configs.items():
            ms[k].append(rounds_ms(launch, a.rounds))
    lines.append({"what": "round_b256", **meta, **{k: stats(v) for k, v in ms.items()}})
    del configs

    # 2. one cv call of 160 models against 160 sequential fits
    K, T = 5, 1
    grid = [(l2, l1) for l2 in (1000.0, 300.0, 100.0, 30.0, 10.0, 3.0, 1.0, 0.3) for l1 in (3.0, 1.0, 0.3, 0.0)]
    fold = (np.arange(n) * 23 // n) % K                    # 23 blocks of rows dealt to the folds in turn
    yh = y[0].cpu().numpy()
    xgblinear.cv(Xc, yh, fold, grid[:1], num_round=2)      # warm-up
    cv_s = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = xgblinear.cv(Xc, yh, fold, grid, num_round=a.rounds)
        torch.cuda.synchronize()
        cv_s.append(time.perf_counter() - t0)
    assert res.heldout.shape == (T, len(grid), K, a.rounds)
    folds_h = [torch.from_numpy((fold != k).astype(np.float32)).to(dev) for k in range(K)]
    seq_lib = parent if parent is not None else lib
    seq_s = sequential_fits(seq_lib, Xc, y[:1], folds_h, a.seq_fits, a.rounds)
    seq_160 = seq_s * 160 / a.seq_fits
    lines.append({"what": "cv_160", **meta, "models": T * len(grid) * K, "cv_s": statistics.median(cv_s),
                  "cv_s_min": min(cv_s), "cv_s_max": max(cv_s), "sequential_fits_timed": a.seq_fits,
                  "sequential_lib": "parent" if parent is not None else "this build", "sequential_s": seq_s,
                  "sequential_160_s": seq_160, "ratio": seq_160 / statistics.median(cv_s)})

    # 3. the rmse launches' share of a cv round
    B = T * len(grid) * K
    m = np.arange(B)
    held = torch.from_numpy(fold).to(dev)[None, :] == torch.from_numpy(m % K).to(dev)[:, None]
    yb, hb, vb = y[:1].expand(B, n).contiguous(), (~held).float().contiguous(), held.float().contiguous()
    hyper = torch.tensor([[HYPER[0], grid[(i // K) % len(grid)][0], grid[(i // K) % len(grid)][1], 0.0] for i in m],
                         dtype=torch.float64, device=dev)
    launch = round_launcher(lib, Xc, yb, hb, B, hyper)
    pred = torch.empty(B, n, device=dev)
    out = torch.zeros(2, B, dtype=torch.float64, device=dev)
    share = []
    for _ in range(a.repeats):
        launch(True)
        launch(False, pred)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.rounds)]
        for e in ev:
            e[0].record()
            launch(False, pred)
            e[1].record()
            for i, wts in enumerate((hb, vb)):
                assert lib.expecto_gblinear_rmse(_lib.dptr(pred), _lib.dptr(yb), n, _lib.dptr(wts), n, n, B,
                                                 _lib.dptr(out[i]), _lib.stream_ptr()) == 0
            e[2].record()
        torch.cuda.synchronize()
        share.append((sum(e[0].elapsed_time(e[1]) for e in ev) / a.rounds, sum(e[1].elapsed_time(e[2]) for e in ev) / a.rounds))
    rnd, rm = [s[0] for s in share], [s[1] for s in share]
    lines.append({"what": "cv_rmse_share", **meta, "models": B, "round": stats(rnd), "two_rmse": stats(rm),
                  "share": statistics.median(rm) / (statistics.median(rm) + statistics.median(rnd))})

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
