"""Drop-in for the part of the reference ``plot_bootstrapped_coefficients.py`` that produces a file
(lines 48-68 and 74-76): the bootstrap standard error of every model coefficient, the z-score of the
main model's coefficient against it, and the input features sorted by ``|z|``.

    python -m expecto_amd.bootstrap_coefficients --bootstrap_model_dir boot --main_model main.save \\
        --feature_clusters_df output_dir/interpret_features/all_feature_clusters.tsv -o out

``--bootstrap_model_dir``, ``--main_model`` and ``-o`` are the reference's.  ``--feature_clusters_df``
replaces its hard-coded ``./output_dir/interpret_features/all_feature_clusters.tsv`` (still the default),
``--max_models`` its ``[:800]``.  The ``<dir>/*/*.save`` files are taken in natural-sort order (digit runs
compare as integers: ``boot2`` before ``boot10``) and read with ``GBLinear.load``; the weights are those of
the text dump (``dump_weights()``: the reference parses the dump's ``%g`` values).  The statistics are one
kernel over the ``[models, coefficients]`` matrix (``expecto_bootstrap_coef_stats``), e.g. the models
``python -m expecto_amd.train --n_bootstrap K`` wrote.

Output: ``input_features_sorted_by_zscore.csv`` (tab-separated as in the reference: the clusters table's
columns plus ``z_score``, index reset) and ``coefficient_stats.tsv`` (``mean``, ``se``, ``z_score``, ``cv``
per coefficient in input order).  The sort is stable on ``|z|`` descending: equal ``|z|`` keep the lower
original row first and NaN goes last (the reference's default quicksort leaves ties in arbitrary order).
The 10 largest coefficients of variation are printed in place of the histograms.  A clusters table whose
row count is not the models' ``num_feature`` is refused.  The SNP-effect arguments the reference parses
and never uses are accepted and ignored.
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import sys

import numpy as np
import pandas as pd

from .xgblinear import GBLinear


def natural_key(s: str):
    """Sort key of natsort's default order for file names: the string split on digit runs, the runs
    compared as integers."""
    return [(0, int(t), '') if t.isdigit() else (1, 0, t) for t in re.split(r'(\d+)', s) if t != '']


def natsorted(names):
    return sorted(names, key=natural_key)


def sort_by_zscore(df: pd.DataFrame, z) -> pd.DataFrame:
    """plot_bootstrapped_coefficients.py:64-67 with a stable sort."""
    df = df.copy()
    df['z_score'] = z
    df['temp'] = np.abs(df['z_score'])
    df = df.sort_values(by='temp', axis=0, ascending=False, kind='stable').reset_index(drop=True)
    return df.drop('temp', axis=1)


def build_parser():
    p = argparse.ArgumentParser(description='Process some integers.')
    p.add_argument('--coorFile', action="store", dest="coorFile", help="accepted and ignored")
    p.add_argument('--geneFile', action="store", dest="geneFile", help="accepted and ignored")
    p.add_argument('--snpEffectFilePattern', action="store", dest="snpEffectFilePattern", help="accepted and ignored")
    p.add_argument('--bootstrap_model_dir', action="store", dest="bootstrap_model_dir", type=str,
                   help='Directory containing bootstrapped models')
    p.add_argument('--main_model', action="store", dest="main_model", type=str,
                   help='Main model fit on X_train without bootstrapping')
    p.add_argument('--belugaFeatures', action="store", dest="belugaFeatures", help="accepted and ignored")
    p.add_argument('--nfeatures', action="store", dest="nfeatures", type=int, default=2002, help="accepted and ignored")
    p.add_argument('--fixeddist', action="store", dest="fixeddist", default=0, type=int, help="accepted and ignored")
    p.add_argument('--maxshift', action="store", dest="maxshift", type=int, default=800, help="accepted and ignored")
    p.add_argument('--batchSize', action="store", dest="batchSize", type=int, default=500, help="accepted and ignored")
    p.add_argument('--splitFlag', action="store_true", default=False, help="accepted and ignored")
    p.add_argument('--splitIndex', action="store", dest="splitIndex", type=int, default=0, help="accepted and ignored")
    p.add_argument('--splitFold', action="store", dest="splitFold", type=int, default=10, help="accepted and ignored")
    p.add_argument('--threads', action="store", dest="threads", type=int, default=16, help="accepted and ignored")
    p.add_argument('--feature_clusters_df', type=str, default='./output_dir/interpret_features/all_feature_clusters.tsv')
    p.add_argument('--max_models', type=int, default=800)
    p.add_argument('-o', action="store", dest="out_dir")
    return p


def run(args) -> dict:
    """Returns {"files", "stats" (mean, se, z, cv), "sorted" (the written frame)}."""
    from .metrics import bootstrap_coef_stats

    os.makedirs(args.out_dir, exist_ok=True)
    model_files = natsorted(glob.glob(f'{args.bootstrap_model_dir}/*/*.save'))[:args.max_models]
    if len(model_files) < 2:
        raise ValueError(f"{len(model_files)} bootstrap models under {args.bootstrap_model_dir}/*/*.save; "
                         "a standard error needs at least 2")
    all_weights = np.vstack([GBLinear.load(f.strip()).dump_weights() for f in model_files])
    weights = GBLinear.load(args.main_model.strip()).dump_weights()
    if weights.shape[0] != all_weights.shape[1]:
        raise ValueError(f"the main model has {weights.shape[0]} coefficients, the bootstrap models "
                         f"{all_weights.shape[1]}")
    input_features_df = pd.read_csv(args.feature_clusters_df, sep='\t', index_col=0)
    if input_features_df.shape[0] != weights.shape[0]:
        raise ValueError(f"{args.feature_clusters_df} has {input_features_df.shape[0]} rows, the models have "
                         f"num_feature = {weights.shape[0]}")

    stats = bootstrap_coef_stats(all_weights, weights)
    out = sort_by_zscore(input_features_df, stats["z"])
    out.to_csv(f'{args.out_dir}/input_features_sorted_by_zscore.csv', sep='\t')
    pd.DataFrame({'mean': stats["mean"], 'se': stats["se"], 'z_score': stats["z"], 'cv': stats["cv"]}).to_csv(
        f'{args.out_dir}/coefficient_stats.tsv', sep='\t')

    k = 10
    top_coeffs_i = np.argsort(stats["cv"])[-k:]
    print(f"Bootstrap models: {len(model_files)}")
    print("Largest coefficients of variation: " + " ".join(str(int(i)) for i in top_coeffs_i[::-1]))
    return {"files": model_files, "stats": stats, "sorted": out}


def main(argv=None):
    from . import _lib

    args = build_parser().parse_args(argv)
    _lib.require_gpu("bootstrap_coefficients")
    return run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
