"""Time the motif scan of ``expecto_amd.query_fimo_for_predictions`` at the size the reference splits into 25
jobs: 40,000 flanks of 61 bp, 2,000 motifs of width 6..30, scanned ``--seq-batch`` sequences at a time
(DESIGN.md section 3 records the figures).

    python tools/pwm_bench.py [--variants 40000] [--motifs 2000] [--seq-batch 8192] [--runs 5] [--cpu-slice 100] \\
        [--cpu-procs 16]

Prints one JSON line: medians over ``--runs`` of the device time (HIP events) of ``pvalue_tables`` and of all
``scan`` calls, and the wall time of a vectorised numpy restatement of the same model on 1 / ``--cpu-slice`` of
the sequences (and of the motifs, for the tables) over ``--cpu-procs`` processes, scaled up for the ratio.
No ``fimo`` binary is timed: none is available to this project.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_CPU = {}


def synth(V, M, L, seed=0):
    from expecto_amd import query_fimo_for_predictions as q
    rng = np.random.RandomState(seed)
    widths = rng.randint(6, 31, M)
    meme = q.Meme(None, [f"ID{m}" for m in range(M)], [f"ALT{m}" for m in range(M)],
                  [rng.dirichlet(np.full(4, 0.4), int(w)) for w in widths], [20.0] * M)
    bg = q.background("nrdb")
    return q.Motifs.from_meme(meme, bg), bg, rng.randint(0, 4, (V, L)).astype(np.uint8)


def numpy_table(s, bg):
    """Rule for rule the device's table, vectorised over the target index (s, bg in code order)."""
    alpha = [0, 2, 1, 3]
    w = s.shape[0]
    old = np.zeros(100 * w + 1)
    old[0] = 1.0
    for i in range(w):
        n_old, n_new = 100 * i + 1, 100 * (i + 1) + 1
        acc = np.zeros(n_new)
        for a in sorted(range(4), key=lambda a: (-int(s[i, alpha[a]]), a)):
            k = np.arange(n_new) - int(s[i, alpha[a]])
            ok = (k >= 0) & (k < n_old)
            acc = acc + np.where(ok, old[np.clip(k, 0, n_old - 1)] * bg[alpha[a]], 0.0)
        old = np.zeros(100 * w + 1)
        old[:n_new] = acc
    pv = np.minimum(np.cumsum(old[::-1])[::-1], 1.0)        # the tail by cumsum: timing only
    pv[0] = 1.0
    return pv


def numpy_scan_motif(m):
    """Best window over position c of motif m in every sequence of the slice: (score, start, strand)."""
    codes, c, pssm, col_ptr = _CPU["codes"], _CPU["c"], _CPU["pssm"], _CPU["col_ptr"]
    s = pssm[col_ptr[m]:col_ptr[m + 1]].astype(np.int32)
    w, (S, L) = s.shape[0], codes.shape
    rc = s[::-1, ::-1]
    best = np.full(S, -1, np.int32)
    start, strand = np.full(S, -1, np.int32), np.zeros(S, np.uint8)
    for p in range(max(0, c - w + 1), min(L - w, c) + 1):
        win = codes[:, p:p + w]
        ok = (win < 4).all(axis=1)
        safe = np.minimum(win, 3)
        plus = s[np.arange(w)[None, :], safe].sum(axis=1)
        minus = rc[np.arange(w)[None, :], safe].sum(axis=1)
        for sc, sd in ((plus, 0), (minus, 1)):
            better = ok & (sc > best)
            best[better], start[better], strand[better] = sc[better], p, sd
    return best, start, strand


def cpu_time(motifs, bg, codes, c, share, procs):
    S = max(1, codes.shape[0] // share)
    Mt = max(1, len(motifs) // share)
    _CPU.update(codes=codes[:S], c=c, pssm=motifs.pssm, col_ptr=motifs.col_ptr)
    bg_code = bg[[0, 2, 1, 3]]
    t0 = time.perf_counter()
    for m in range(Mt):
        numpy_table(motifs.pssm[motifs.col_ptr[m]:motifs.col_ptr[m + 1]].astype(np.int64), bg_code)
    t1 = time.perf_counter()
    with Pool(procs) as pool:                   # forked before the device is opened
        t2 = time.perf_counter()
        pool.map(numpy_scan_motif, range(len(motifs)), chunksize=8)
        t3 = time.perf_counter()
    return {"cpu_tables_ms": 1e3 * (t1 - t0), "cpu_tables_motifs": Mt, "cpu_scan_ms": 1e3 * (t3 - t2), "cpu_scan_sequences": S,
            "cpu_procs": procs}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--variants", type=int, default=40000)
    ap.add_argument("--motifs", type=int, default=2000)
    ap.add_argument("--length", type=int, default=61)
    ap.add_argument("--seq-batch", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cpu-slice", type=int, default=100)
    ap.add_argument("--cpu-procs", type=int, default=16)
    a = ap.parse_args()
    motifs, bg, codes = synth(a.variants, a.motifs, a.length)
    c = a.length // 2
    out = {"V": a.variants, "M": a.motifs, "L": a.length, "seq_batch": a.seq_batch, "columns": int(motifs.col_ptr[-1])}
    if a.cpu_slice > 0:
        out.update(cpu_time(motifs, bg, codes, c, a.cpu_slice, a.cpu_procs))
    import torch

    from expecto_amd import query_fimo_for_predictions as q
    if not torch.cuda.is_available():
        raise SystemExit("pwm_bench needs a GPU: a CPU run gives no time")
    d_codes = torch.from_numpy(codes).cuda()
    tables = q.pvalue_tables(motifs, bg)                          # warm-up: code objects, allocator
    q.scan(d_codes[:a.seq_batch], c, motifs, tables)
    torch.cuda.synchronize()
    t_tab, t_scan = [], []
    for _ in range(a.runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        tables = q.pvalue_tables(motifs, bg)
        ev[1].record()
        torch.cuda.synchronize()
        ev[2].record()
        for s0 in range(0, a.variants, a.seq_batch):
            res = q.scan(d_codes[s0:s0 + a.seq_batch], c, motifs, tables)
        ev[3].record()
        torch.cuda.synchronize()
        t_tab.append(ev[0].elapsed_time(ev[1]))
        t_scan.append(ev[2].elapsed_time(ev[3]))
        del res
    out.update(runs=a.runs, tables_ms=round(float(np.median(t_tab)), 3), scan_ms=round(float(np.median(t_scan)), 3),
               tables_ms_all=[round(t, 3) for t in t_tab], scan_ms_all=[round(t, 3) for t in t_scan])
    if a.cpu_slice > 0:
        out["scan_ratio_cpu_scaled_over_gpu"] = round(out["cpu_scan_ms"] * a.variants / out["cpu_scan_sequences"] / out["scan_ms"], 1)
        out["tables_ratio_cpu_scaled_over_gpu"] = round(out["cpu_tables_ms"] * a.motifs / out["cpu_tables_motifs"] / out["tables_ms"], 1)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)


if __name__ == "__main__":
    main()
