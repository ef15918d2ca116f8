"""Golden stdout of the reference ``cluster_analysis_with_fimo.py`` CLI on two small inputs.

Run from the repo root on a CPU machine (needs pandas, scipy and /root/reference; neither the
reference nor scipy is read by the GPU tests):
    python tests/golden/make_golden_fimo.py

Writes tests/golden/fimo/<case>/ for the cases of ``enrich_ref.fixture``: the three inputs
(``cluster_contribs.tsv``, ``rsat_clusters.tsv``, ``fimo.tsv``) and ``stdout.txt`` of the unmodified
reference script, run in a temporary directory.  tests/golden/stubs_fimo goes ahead of
tests/golden/stubs_contribs on PYTHONPATH: the latter's pyplot lacks ``plot`` / ``xlabel`` / ``ylim``,
which this script calls.  ``main`` also gets ``stdout_rank_int.txt``, the same run with ``--rank_int``.

The inputs: 12 rows over 9 rsids and 4 genes with 15 leading columns (the reference reads the cluster
columns at position 15), 25 clusters of 3 motifs plus ``cluster_-1`` (so T = 26 - 20 = 6), and a FIMO
table in which every motif occurs, some rows lie outside the +-30 bp window or above the p-value
threshold, one rsid has no row and one sequence belongs to no variant.  No row has two equal
magnitudes (asserted by the recipe): pandas' ``sort_values`` is not stable, so ties are outside what
the reference defines.  ``shared``: one motif name in two clusters.

Also ``hypergeom_exact.json``: for every quadruple of ``enrich_ref.sf_quadruples()`` the exact upper tail
to 40 significant digits (``enrich_ref.exact_sf_digits``; a couple of minutes of big-integer arithmetic).
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import sys
import tempfile

GOLD = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, GOLD)
sys.path.insert(0, os.path.dirname(GOLD))
import enrich_ref  # noqa: E402
from make_golden_predict import REF  # noqa: E402

DST = os.path.join(GOLD, "fimo")
STUBS = os.path.join(GOLD, "stubs_fimo") + ":" + os.path.join(GOLD, "stubs_contribs")
NAMES = ("cluster_contribs.tsv", "rsat_clusters.tsv", "fimo.tsv")


def run_reference(work, extra=()):
    env = dict(os.environ, PYTHONPATH=STUBS + ":" + REF, OMP_NUM_THREADS="8", PYTHONWARNINGS="ignore")
    out = subprocess.run([sys.executable, os.path.join(REF, "cluster_analysis_with_fimo.py"),
                          "--cluster_contribs_file", NAMES[0], "--rsat_clusters_file", NAMES[1],
                          "--fimo_out_file", NAMES[2], *extra, "-o", "out"], cwd=work, env=env, capture_output=True,
                         text=True)
    if out.returncode:
        sys.stderr.write(out.stderr)
        raise SystemExit(out.returncode)
    return out.stdout


def main():
    for case in ("main", "shared"):
        work = tempfile.mkdtemp(prefix="expecto_golden_fimo_")
        dst = os.path.join(DST, case)
        os.makedirs(dst, exist_ok=True)
        for name, text in zip(NAMES, enrich_ref.fixture(case)):
            for root in (work, dst):
                with open(os.path.join(root, name), "w") as f:
                    f.write(text)
        with open(os.path.join(dst, "stdout.txt"), "w") as f:
            f.write(run_reference(work))
        if case == "main":
            with open(os.path.join(dst, "stdout_rank_int.txt"), "w") as f:
                f.write(run_reference(work, ("--rank_int",)))
        shutil.rmtree(work)
    with open(os.path.join(DST, "hypergeom_exact.json"), "w") as f:
        json.dump([[*q, enrich_ref.exact_sf_digits(*q)] for q in enrich_ref.sf_quadruples()], f, indent=0)
    print("cluster_analysis_with_fimo.py golden outputs written to", DST)


if __name__ == "__main__":
    main()
