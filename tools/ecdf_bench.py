"""Time the empirical significance step at the size of a real run: n = 100,000 query variants against a
background of B = 100,000 variants, C = nc = 2002 marks, on seeded effects (DESIGN.md "Empirical significance"
records the figures).

    python tools/ecdf_bench.py [--n 100000] [--B 100000] [--marks 2002] [--runs 5] [--rounds 3] [--timeout 300]

Two things are timed on the same device and the same tensors, with HIP events after warm runs:
  kernel    expecto_ecdf_tail_counts + expecto_ecdf_summary;
  baseline  the plumbing alternative: torch.searchsorted on the [C, B] table with the transposed queries, plus
            torch reductions for the four summaries (its sums are in torch's order, not the stated one).
They alternate for ``--rounds`` rounds; every step is a child process of its own under ``--timeout`` seconds, and
the first step that fails ends the run.  Prints one JSON line: the median over runs of every step, the medians
over rounds, the ratio baseline / kernel and the achieved bytes/s of the x read and the ge write.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(a):
    """(background, x) on the device: seeded effects with a per-mark scale, as chromatin effects have."""
    import torch

    from expecto_amd import significance as sg
    g = torch.Generator(device="cuda").manual_seed(1234)
    scale = 10.0 ** (torch.rand((1, a.marks), generator=g, device="cuda") * 3 - 4)
    bg = sg.build_background(torch.randn((a.B, a.marks), generator=g, device="cuda") * scale)
    x = torch.randn((a.n, a.marks), generator=g, device="cuda") * scale
    return bg, x


def timed(fn, runs):
    import torch
    fn()                                                        # warm-up: code objects, allocator
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def step(a):
    import torch

    from expecto_amd import significance as sg
    if not torch.cuda.is_available():
        raise SystemExit("ecdf_bench needs a GPU: a CPU run gives no time")
    bg, x = inputs(a)
    B, k_alpha = bg.n, int(np.floor(0.01 * (bg.n + 1)))
    out = {"step": a.step}
    if a.step == "kernel":
        out["tail_counts_ms"] = timed(lambda: sg.tail_counts(bg, x), a.runs)
        out["total_ms"] = timed(lambda: sg.score(bg, x, alpha=0.01), a.runs)
    else:
        lut = bg.lut()

        def baseline():
            lb = torch.searchsorted(bg.sorted, x.abs().T.contiguous(), right=False)      # [C, n] int64
            ge = (B - lb).T
            nlog = lut[ge]
            return ge, nlog.mean(1), nlog.max(1).values, ge.argmin(1), (ge < k_alpha).sum(1)
        out["total_ms"] = timed(baseline, a.runs)
        ge = sg.tail_counts(bg, x)                              # the two agree on the counts
        out["counts_equal"] = bool(torch.equal(baseline()[0].to(torch.int32), ge))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--B", type=int, default=100000)
    ap.add_argument("--marks", type=int, default=2002)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    ap.add_argument("--step", choices=("kernel", "baseline"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a)
    res = {"kernel": [], "baseline": [], "tail_counts": []}
    equal = True
    for _ in range(a.rounds):
        for name in ("kernel", "baseline"):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--n", str(a.n), "--B", str(a.B), "--marks", str(a.marks), "--runs", str(a.runs)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:                               # a fault, an abort or the time limit: stop here
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"step {name} ended with status {p.returncode}; nothing more is started")
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[name].append(float(np.median(r["total_ms"])))
            if name == "kernel":
                res["tail_counts"].append(float(np.median(r["tail_counts_ms"])))
            else:
                equal = equal and r["counts_equal"]
    k, b, t = (float(np.median(res[x])) for x in ("kernel", "baseline", "tail_counts"))
    nbytes = 4.0 * a.n * a.marks
    print(json.dumps({
        "n": a.n, "B": a.B, "marks": a.marks, "runs": a.runs, "rounds": a.rounds,
        "kernel_ms_rounds": [round(v, 3) for v in res["kernel"]],
        "baseline_ms_rounds": [round(v, 3) for v in res["baseline"]],
        "tail_counts_ms_rounds": [round(v, 3) for v in res["tail_counts"]],
        "kernel_ms": round(k, 3), "baseline_ms": round(b, 3), "tail_counts_ms": round(t, 3),
        "ratio_baseline_over_kernel": round(b / k, 2),
        "x_read_GBps": round(nbytes / (t * 1e-3) / 1e9, 1), "ge_write_GBps": round(nbytes / (t * 1e-3) / 1e9, 1),
        "counts_equal": equal}), flush=True)


if __name__ == "__main__":
    main()
