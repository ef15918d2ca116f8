"""Time the saturation-mutagenesis scoring at one gene's shape (DESIGN.md "Saturation mutagenesis"
records the figures): 2000 positions (6000 SNV slots), 9 shifts, 2002 marks, 218 models and 1 model.

    python tools/ism_bench.py [--positions 2000] [--models 218,1] [--rounds 5] [--chain-rounds 3] [--no-gene]

Per model count, on the same device buffers and in alternating rounds after a warm-up of both:
(a) ``expecto_ism_score``, the fused kernel; (b) the chain of entry points it replaces
(``expecto_fwd_rc_average`` and ``expecto_variant_reduce_lut`` per allele, ``expecto_gblinear_predict`` per
allele and model), whose outputs it must equal bit for bit (checked once).  Times are HIP-event
milliseconds; the spread is the min and max over the rounds.  Then one gene end to end through
``mutagenesis.saturation`` on a synthetic genome with seeded Beluga weights, its device time split into the
forward and the scoring.  Prints one JSON line per measurement; needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NFEAT = 2002
SHIFTS = [0, -200, -400, -600, -800, 200, 400, 600, 800]


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "rounds": len(ms)}


def score_shapes(args):
    import torch
    from expecto_amd import _lib
    from expecto_amd import mutagenesis as mg
    from expecto_amd.features import decay_table
    from expecto_amd.xgblinear import GBLinear

    lib = _lib.load()
    P, S = args.positions, len(SHIFTS)
    n = 3 * P
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.randn((2, 2, S, n, NFEAT), device="cuda", generator=g)
    y[:, 0] = y[:, 0, :, 0::3].repeat_interleave(3, dim=2)          # one ref window per position
    dist = np.arange(-(P // 2), P - P // 2, dtype=np.int64)
    dist_d = torch.from_numpy(np.repeat(dist, 3)).cuda()
    sp = torch.ones(n, dtype=torch.uint8, device="cuda")
    valid = torch.ones(n, dtype=torch.uint8, device="cuda")
    shifts_d = torch.tensor(SHIFTS, dtype=torch.int32, device="cuda")
    lut = torch.from_numpy(decay_table(dist, np.ones(P, bool), SHIFTS)).cuda()
    keep = np.arange(NFEAT, dtype=np.int32)
    cols = torch.arange(10 * NFEAT, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    avg = torch.empty((S * n, NFEAT), dtype=torch.float32, device="cuda")
    feat = torch.empty((n, 10 * NFEAT), dtype=torch.float64, device="cuda")
    st = _lib.stream_ptr()
    ya = [y[:, a].contiguous() for a in range(2)]   # an allele's rows of both strands as one block (not timed)
    for M in args.models:
        models = [GBLinear(rng.normal(0, 0.05, (10 * NFEAT, 1)).astype(np.float32),
                           rng.normal(0, 1, 1).astype(np.float32), 2.0) for _ in range(M)]
        bank = mg.ModelBank(models, keep)
        wm = bank.w.t().contiguous()                                  # [M, 10 nk]: the chain's per-model vectors
        init = bank.init.cpu().numpy()
        fused = None
        chain = torch.empty((2, M, n), dtype=torch.float32, device="cuda")

        def run_fused():
            nonlocal fused
            fused = mg.score_slots(y, dist_d, True, shifts_d, lut, bank, valid, fused)

        def run_chain():
            for a in range(2):
                _lib.check(lib.expecto_fwd_rc_average(_lib.dptr(ya[a]), S * n, NFEAT, _lib.dptr(avg), st), "avg")
                _lib.check(lib.expecto_variant_reduce_lut(_lib.dptr(avg), _lib.dptr(dist_d), _lib.dptr(sp),
                                                          _lib.dptr(shifts_d), S, n, NFEAT, _lib.dptr(lut),
                                                          int(lut.shape[1]), _lib.dptr(feat), st), "reduce")
                for m in range(M):
                    _lib.check(lib.expecto_gblinear_predict(_lib.dptr(feat), n, 10 * NFEAT, _lib.dptr(cols), 10 * NFEAT,
                                                            _lib.dptr(wm[m]), float(init[m]), _lib.dptr(chain[a, m]),
                                                            st), "gblinear")

        run_fused()
        run_chain()
        torch.cuda.synchronize()
        alt_pred, ref_pred, sed = fused
        same = bool(torch.equal(alt_pred.view(torch.int32), chain[1].view(torch.int32)) and
                    torch.equal(ref_pred.view(torch.int32), chain[0][:, 0::3].contiguous().view(torch.int32)) and
                    torch.equal(sed, chain[1].double() - chain[0].double()))
        tf, tc = [], []
        for r in range(max(args.rounds, args.chain_rounds)):           # alternating rounds
            if r < args.rounds:
                tf.append(timed(run_fused))
            if r < args.chain_rounds:
                tc.append(timed(run_chain))
        # bytes the fused kernel has to move: the four rows of a position (the ref rows of its first slot, three
        # alt rows) of both strands and every shift once, the weights once, the outputs; and the bytes its
        # workgroups stream (each position reads every model's weights, served by L2 / the Infinity Cache)
        rows_b = P * 4 * 2 * S * NFEAT * 4
        w_b = 10 * NFEAT * M * 4
        out_b = M * (n * 12 + P * 4)
        f = stats(tf)
        print(json.dumps({
            "what": "ism_score", "positions": P, "shifts": S, "marks": NFEAT, "models": M, "bitwise_equal_to_chain": same,
            "fused": f, "chain": stats(tc),
            "fused_compulsory_bytes": rows_b + w_b + out_b, "fused_streamed_bytes": rows_b * 10 + w_b * P + out_b,
            "fused_compulsory_TBps": (rows_b + w_b + out_b) / f["median_ms"] * 1e-9,
            "fused_streamed_TBps": (rows_b * 10 + w_b * P + out_b) / f["median_ms"] * 1e-9,
            "fused_f32_ops_per_s": 2.0 * 4 * 10 * NFEAT * M * P / f["median_ms"] * 1e3}), flush=True)
        del bank, wm, chain, fused


def one_gene(args):
    import torch
    from expecto_amd import beluga, synthetic
    from expecto_amd import mutagenesis as mg
    from expecto_amd.genome import DeviceGenome, Fasta
    from expecto_amd.pipeline import VariantPipeline
    from expecto_amd.xgblinear import GBLinear

    fa = Fasta.from_dict(synthetic.genome_bytes(n_contigs=1, contig_len=200000, seed=7))
    eng = beluga.seeded(0, gain=math.sqrt(6.0), max_batch=args.max_batch).cuda().engine()
    pipe = VariantPipeline(eng, fa, DeviceGenome(fa))
    rng = np.random.default_rng(2)
    M = max(args.models)
    bank = mg.ModelBank([GBLinear(rng.normal(0, 0.05, (10 * NFEAT, 1)).astype(np.float32),
                                  rng.normal(0, 1, 1).astype(np.float32), 2.0) for _ in range(M)],
                        np.arange(NFEAT, dtype=np.int32))
    half = args.positions // 2
    runs = []
    for r in range(1 + args.gene_rounds):                              # the first run is the warm-up
        t = {}
        ms = timed(lambda: mg.saturation(pipe, bank, "chr1", 100000, "+", half, args.positions - half, 800,
                                         args.positions_per_batch, timing=t))
        if r:
            runs.append((ms, t["forward_ms"], t["score_ms"]))
    tot, fwd, sc = (stats([x[i] for x in runs]) for i in range(3))
    print(json.dumps({"what": "saturation", "positions": args.positions, "models": M, "maxshift": 800,
                      "positions_per_batch": args.positions_per_batch, "precision": "f16x3", "total": tot, "forward": fwd,
                      "score": sc}), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--positions", type=int, default=2000)
    p.add_argument("--models", type=lambda s: [int(x) for x in s.split(",")], default=[218, 1])
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--chain-rounds", type=int, default=3, dest="chain_rounds")
    p.add_argument("--gene-rounds", type=int, default=3, dest="gene_rounds")
    p.add_argument("--positions-per-batch", type=int, default=512, dest="positions_per_batch")
    p.add_argument("--max-batch", type=int, default=8192, dest="max_batch")
    p.add_argument("--no-gene", action="store_true", dest="no_gene")
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("tools/ism_bench.py needs a GPU (HIP)")
    score_shapes(args)
    if not args.no_gene:
        one_gene(args)


if __name__ == "__main__":
    main()
