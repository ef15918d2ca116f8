"""Golden outputs of the reference ``interpret_features_grouped.py`` CLI (``all_feature_clusters.tsv``,
``cluster_sizes.tsv`` and its stdout).

Run from the repo root (needs /root/reference with scipy, scikit-learn, joblib and tqdm installed;
never read at test time):
    python tests/golden/make_golden_interpret.py

The reference script runs unmodified, with tests/golden/stubs on PYTHONPATH for the xgboost /
matplotlib / seaborn imports it never uses.  Its input is ``tests/ward_ref.interpret_inputs()``: a
seeded [40 genes, 20020] matrix (the script hard-codes 2002 marks) whose genes lie on chr1, chr2,
chr8, chrX and chrY, with one ``rRNA`` row and, with ``--pseudocount 0``, one zero expression value
among the training genes, so the type filter, the train split and the finiteness mask all drop
rows: 22 training genes, 2002 points of 220 dimensions.  The test regenerates the matrix from the
same function; only the two small CSVs are stored.

Writes tests/golden/interpret_features/: geneanno.csv, geneexp.csv (inputs), stdout.txt,
all_feature_clusters.tsv, cluster_sizes.tsv (outputs).  The features table is
tests/golden/predict_sed/deepsea_beluga_2002_features.tsv.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

GOLD = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, GOLD)
sys.path.insert(0, os.path.dirname(GOLD))
from make_golden_predict import REF, STUBS  # noqa: E402
from ward_ref import write_interpret_inputs  # noqa: E402

DST = os.path.join(GOLD, "interpret_features")
FEATURES_TSV = os.path.join(GOLD, "predict_sed", "deepsea_beluga_2002_features.tsv")
TARGET_INDEX = 1


def main():
    work = tempfile.mkdtemp(prefix="expecto_golden_interpret_")
    os.makedirs(DST, exist_ok=True)
    x_path, anno_path, exp_path = write_interpret_inputs(work)
    env = dict(os.environ, PYTHONPATH=STUBS + ":" + REF, OMP_NUM_THREADS="8")
    out = subprocess.run([sys.executable, os.path.join(REF, "interpret_features_grouped.py"),
                          "--belugaFeatures", FEATURES_TSV, "--targetIndex", str(TARGET_INDEX), "--expFile", exp_path,
                          "--inputFile", x_path, "--annoFile", anno_path, "--pseudocount", "0", "--out_dir", "iout"],
                         cwd=work, env=env, capture_output=True, text=True)
    if out.returncode:
        sys.stderr.write(out.stderr)
        raise SystemExit(out.returncode)
    with open(os.path.join(DST, "stdout.txt"), "w") as f:
        f.write(out.stdout)
    for t in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
        shutil.copy(os.path.join(work, "iout", t), os.path.join(DST, t))
    for p in (anno_path, exp_path):
        shutil.copy(p, os.path.join(DST, os.path.basename(p)))
    shutil.rmtree(work)
    print("interpret_features_grouped.py golden outputs written to", DST)


if __name__ == "__main__":
    main()
