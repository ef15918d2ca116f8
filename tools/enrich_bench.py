"""Time ``python -m expecto_amd.cluster_analysis_with_fimo`` on a synthetic input of the size the reference
was written for, and split the time into host draw, upload, ``expecto_cluster_enrich`` and
``expecto_hypergeom_sf`` (DESIGN.md section 3 records the figures).

    python tools/enrich_bench.py [--variants 5000] [--clusters 110] [--motifs 800] [--matches 40] \\
        [--permutations 1 1000] [--runs 5] [--dir DIR]

Prints one JSON line per permutation count: the medians over ``--runs`` runs of the wall time of
``run()`` (files read, device calls, files written; the process start and imports are not in it) and of
its parts.  ``--write-only`` writes the input files and exits (for a CPU run of another program on them).
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(root, V, C, M, per_variant, seed=0, leading=15):
    """cluster_contribs.tsv (``leading`` columns before the clusters), rsat_clusters.tsv (M motifs dealt
    over C clusters, plus cluster_-1) and fimo.tsv (about ``per_variant`` matching rows per variant, every
    motif at least once)."""
    rng = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    motifs = [f"MOTIF{m:05d}" for m in range(M)]
    head = [str(i) for i in range(leading - 7)] + ["dist", "gene", "strand", "REF", "ALT", "SED", "SED_PROPORTION"]
    contrib = rng.standard_normal((V, C + 1))
    sed = rng.standard_normal(V) * 0.01
    with open(os.path.join(root, "cluster_contribs.tsv"), "w") as f:
        f.write("\t".join(["index", *head, *[f"cluster_{c + 1}" for c in range(C)], "cluster_-1"]) + "\n")
        for v in range(V):
            lead = [f"f{i}" for i in range(leading - 7)]
            lead[2] = f"rs{v}"
            lead += [str(v % 997), f"ENSG{v % 400:05d}", "+", "1.0", "1.1", repr(float(sed[v])), repr(float(abs(sed[v]) / 2))]
            f.write("\t".join([str(v), *lead, *[repr(float(x)) for x in contrib[v]]]) + "\n")
    with open(os.path.join(root, "rsat_clusters.tsv"), "w") as f:
        for c in range(C):
            f.write(f"cluster_{c + 1}\t{','.join(motifs[c::C])}\n")
        f.write("cluster_-1\tUNPLACED\n")
    with open(os.path.join(root, "fimo.tsv"), "w") as f:
        f.write("# motif_id\tmotif_alt_id\tsequence_name\tstart\tstop\tstrand\tscore\tp-value\tq-value\tmatched_sequence\n")
        for v in range(V):
            pick = rng.choice(M, per_variant, replace=False)
            if v < M:
                pick[0] = v
            for m in set(pick.tolist()):
                f.write(f"ID{m}\t{motifs[m]}\trs{v}\t25\t36\t+\t12.5\t1e-06\t0.5\tACGTACGTACGT\n")
    return root


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--variants", type=int, default=5000)
    ap.add_argument("--clusters", type=int, default=110)
    ap.add_argument("--motifs", type=int, default=800)
    ap.add_argument("--matches", type=int, default=40)
    ap.add_argument("--permutations", type=int, nargs="+", default=[1, 1000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--write-only", action="store_true")
    a = ap.parse_args()
    root = synth(a.dir or tempfile.mkdtemp(prefix="enrich_bench_"), a.variants, a.clusters, a.motifs, a.matches)
    if a.write_only:
        print(root)
        return
    import torch

    from expecto_amd import cluster_analysis_with_fimo as caf
    if not torch.cuda.is_available():
        raise SystemExit("enrich_bench needs a GPU: a CPU run gives no time")
    base = ["--cluster_contribs_file", f"{root}/cluster_contribs.tsv", "--rsat_clusters_file", f"{root}/rsat_clusters.tsv",
            "--fimo_out_file", f"{root}/fimo.tsv", "-o", f"{root}/out"]
    caf.run(caf.build_parser().parse_args(base), out=io.StringIO())           # warm-up: code objects, allocator
    for P in a.permutations:
        rows = []
        for _ in range(a.runs):
            timings = {}
            t0 = time.perf_counter()
            caf.run(caf.build_parser().parse_args(base + ["--n_permutations", str(P)]), out=io.StringIO(), timings=timings)
            torch.cuda.synchronize()
            timings["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            rows.append(timings)
            print(json.dumps({"P": P, "run": len(rows), **{k: round(v, 3) for k, v in timings.items()}}), flush=True)
        med = {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}
        print(json.dumps({"V": a.variants, "C": a.clusters, "M": a.motifs, "matches_per_variant": a.matches, "P": P,
                          "runs": a.runs, "median": med}), flush=True)


if __name__ == "__main__":
    main()
