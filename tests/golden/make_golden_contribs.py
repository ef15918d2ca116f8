"""Golden outputs of the reference ``predict_by_cluster_rsat.py`` CLI (the sed tables plus
``sed_sorted_by_proportion_with_contribs.tsv``, ``cluster_contribs.tsv``, ``rsat_clusters.tsv``).

Run from the repo root (needs /root/reference; never read at test time):
    python tests/golden/make_golden_contribs.py

Inputs are the fixtures of make_golden.py, as in make_golden_predict.py: the reference
chromatin.py outputs for shifts 0/-200/200 (chromatin.npz) and the coordinate / gene-association
rows (predict_features.npz).  The reference script runs unmodified in a temporary working
directory that holds synthetic ``resources/Lambert-hgnc-symbol-check.csv`` and
``resources/beluga_hgnc_mapping.csv`` (the script needs ``--intersect_with_lambert``: only then
does cluster_utils.get_keep_mask return the HGNC table it indexes).  They keep 40 marks:

    Max (9, mapped to MAX), c-Jun (9, JUN), c-Fos (8; two mapping rows, the "Approved symbol"
    one gives FOS), ZNF274 (7) and STAT3 (7), both unmapped.

The synthetic rsat tab has MAX in clusters 1 and 2 (one name lower case, one with another
``_`` suffix), JUN and FOS in 2, ZNF274 in 3, TP53 (no kept mark) in 4 and STAT3 in none
(``cluster_-1``).  tests/golden/stubs_contribs goes ahead of tests/golden/stubs on PYTHONPATH:
its xgboost adds ``get_dump()``, its matplotlib accepts the plotting calls.  --batchSize 3 gives
3 batches over the 7 rows.

Writes tests/golden/predict_by_cluster/: the inputs (model.save, clusters_motif_names.tab,
resources/*.csv) and the outputs (stdout.txt, sed.csv, sed_sorted_by_magnitude.tsv,
sed_sorted_by_proportion.tsv, sed_sorted_by_proportion_with_contribs.tsv, cluster_contribs.tsv,
rsat_clusters.tsv).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, GOLD)
from make_golden_predict import FEATURES_TSV, REF, STUBS, write_model  # noqa: E402

STUBS_CONTRIBS = os.path.join(GOLD, "stubs_contribs")
DST = os.path.join(GOLD, "predict_by_cluster")
N_KEEP = 40
OUTPUTS = ("sed.csv", "sed_sorted_by_magnitude.tsv", "sed_sorted_by_proportion.tsv",
           "sed_sorted_by_proportion_with_contribs.tsv", "cluster_contribs.tsv", "rsat_clusters.tsv")

LAMBERT = "\n".join([",Input,Match type,Approved symbol", "0,MAX,Approved symbol,MAX", "1,JUN,Approved symbol,JUN",
                     "2,FOS,Approved symbol,FOS", "3,ZNF274,Approved symbol,ZNF274",
                     "4,STAT3,Approved symbol,STAT3", "5,TP53,Approved symbol,TP53"]) + "\n"
MAPPING = "\n".join(["Input,Match type,Approved symbol", "Max,Approved symbol,Max", "c-Jun,Alias symbol,Jun",
                     "c-Fos,Previous symbol,FOSB", "c-Fos,Approved symbol,FOS", "GR,Unmatched,"]) + "\n"
RSAT_TAB = "\n".join(["cluster_1\tmax_HUMAN.H11MO.0.A,MYC_HUMAN.H11MO.0.A",
                      "cluster_2\tJUN_HUMAN.H11MO.0.A,FOS_HUMAN.H11MO.0.A,Max_MOUSE.H11MO.0.A",
                      "cluster_3\tZNF274_HUMAN.H11MO.0.C",
                      "cluster_4\tP53_HUMAN.H11MO.0.A,TP53_HUMAN.H11MO.1.A"]) + "\n"


def main():
    chrom = np.load(os.path.join(GOLD, "chromatin.npz"))
    feats = np.load(os.path.join(GOLD, "predict_features.npz"))
    work = tempfile.mkdtemp(prefix="expecto_golden_contribs_")
    os.makedirs(os.path.join(work, "out"))
    os.makedirs(os.path.join(work, "resources"))
    os.makedirs(os.path.join(DST, "resources"), exist_ok=True)
    for s in (0, -200, 200):
        np.savez(os.path.join(work, "out", f"snps.shift_{s}.diff.h5.npz"),
                 **{k: chrom[f"{k}_{s}"] for k in ("diff", "ref", "alt")})
    with open(os.path.join(work, "coor.vcf"), "w") as f:
        f.write("##fileformat=VCFv4.3\n")
        for r in feats["coor_rows"]:
            f.write(str(r) + "\n")
    with open(os.path.join(work, "genes.tsv"), "w") as f:
        for r in feats["gene_rows"]:
            f.write(str(r) + "\n")
    for name, text in (("resources/Lambert-hgnc-symbol-check.csv", LAMBERT),
                       ("resources/beluga_hgnc_mapping.csv", MAPPING), ("clusters_motif_names.tab", RSAT_TAB)):
        for root in (work, DST):
            with open(os.path.join(root, name), "w") as f:
                f.write(text)
    model = os.path.join(DST, "model.save")
    write_model(model, 10 * N_KEEP, 13)
    env = dict(os.environ, PYTHONPATH=STUBS_CONTRIBS + ":" + STUBS + ":" + REF, OMP_NUM_THREADS="8")
    out = subprocess.run([sys.executable, os.path.join(REF, "predict_by_cluster_rsat.py"), "--model_save_file", model,
                          "--belugaFeatures", FEATURES_TSV, "--coorFile_chromatin", os.path.join(work, "coor.vcf"),
                          "--geneFile", os.path.join(work, "genes.tsv"),
                          "--snpEffectFilePattern", os.path.join(work, "out", "snps.shift_SHIFT.diff.h5"),
                          "--rsat_clusters_tab", os.path.join(work, "clusters_motif_names.tab"),
                          "--intersect_with_lambert", "--maxshift", "200", "--batchSize", "3", "-o", "pout"],
                         cwd=work, env=env, capture_output=True, text=True)
    if out.returncode:
        sys.stderr.write(out.stderr)
        raise SystemExit(out.returncode)
    with open(os.path.join(DST, "stdout.txt"), "w") as f:
        f.write(out.stdout)
    for t in OUTPUTS:
        shutil.copy(os.path.join(work, "pout", t), os.path.join(DST, t))
    shutil.rmtree(work)
    print("predict_by_cluster_rsat.py golden outputs written to", DST)


if __name__ == "__main__":
    main()
