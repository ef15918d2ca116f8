"""Drop-in for the reference ``predict_by_cluster_rsat.py`` and ``predict_by_cluster.py`` CLIs:
which chromatin marks, and which clusters of marks, drive a variant's predicted expression
change.

    python -m expecto_amd.predict_by_cluster --model_save_file M.save [M2.save ...] \\
        --belugaFeatures features.tsv --coorFile_chromatin snps_hg19.vcf --geneFile closestgene.tsv \\
        --snpEffectFilePattern out/snps.shift_SHIFT.diff.h5 --intersect_with_lambert \\
        --rsat_clusters_tab clusters_motif_names.tab [--maxshift 800] -o out_dir

Arguments are those of ``predict_by_cluster_rsat.py:15-57`` plus ``--feature_clusters_df``
(``predict_by_cluster.py:25-26``).  The rows (duplicate masking, gene repeats, dist, strand) and
REF / ALT / SED come from :mod:`expecto_amd.predict`, in the reference's float32 arithmetic.  The
interpretation step (``interpret_model``, ``interpret_model_with_clusters[_rsat]``;
``predict_by_cluster_rsat.py:105-144``, ``predict_by_cluster.py:73-109``) is one device pass
over the chromatin effects for all models: :func:`expecto_amd.features.variant_contributions`
(``expecto_variant_contrib``), which never builds the ``[n, 20020]`` feature matrices.  It runs
in the reference's batches of ``--batchSize`` rows and asks only for the two proportion tensors
the files hold, so device memory is ``models x batchSize x (marks + clusters)`` float64.

* ``--rsat_clusters_tab`` (``predict_by_cluster_rsat.py:74-102``; needs
  ``--intersect_with_lambert``, as the reference does, for the HGNC assay names): an assay
  belongs to every rsat cluster whose upper-cased motif names, cut at the first ``_``, hold it,
  else to ``cluster_-1``.  Cluster columns appear in the order the kept marks first reach them.
  Writes ``sed.csv``, ``sed_sorted_by_magnitude.tsv``, ``sed_sorted_by_proportion.tsv``,
  ``sed_sorted_by_proportion_with_contribs.tsv`` (columns ``Assay/Cell type``),
  ``cluster_contribs.tsv`` and ``rsat_clusters.tsv`` (with the ``cluster_-1`` row).
* ``--feature_clusters_df`` (``predict_by_cluster.py:64-65,102-107``): column ``cluster`` of
  ``all_feature_clusters.tsv`` (``interpret_features.py:124-128``), one row per kept mark or one
  per (mark, coeff_idx); a mark's ten rows must carry one label, since a cluster here is a set
  of marks.  Clusters are the sorted labels, columns ``cluster_0..``; contribution columns are
  ``Assay type/Assay/Cell type``; the files are ``sed.csv`` and ``.csv`` for the other four
  (``predict_by_cluster.py:306-330``).

Stdout lines are the reference's.  Not in the reference: ``--model_save_file`` takes several
files; with more than one, each model's files go to ``<out_dir>/<model file stem>/``.  The bar
plots of ``predict_by_cluster_rsat.py:395-419`` (``cluster_figures/``) are left out.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import pandas as pd
import torch

from . import _lib, predict
from .features import variant_contributions
from .pipeline import shift_order
from .xgblinear import GBLinear

MOTIF_NOT_FOUND_CLUSTER_ID = -1


def build_parser():
    p = predict.build_parser()
    for a in p._actions:
        if a.dest == "model_save_file":
            a.nargs = "+"
            a.help = "Save file(s) containing the model(s) to use for predictions"
    p.add_argument('--feature_clusters_df', action="store", dest="feature_clusters_df",
                   help="tsv file for clustered features")
    return p


def rsat_clusters(tab_path: str, assays):
    """predict_by_cluster_rsat.py:74-102.  Returns (per-assay lists of cluster ids, the tab table
    indexed by cluster name with the ``cluster_-1`` row added)."""
    rsat_clusters_df = pd.read_csv(tab_path, sep='\t', header=None)
    sets = [set(m.split("_")[0] for m in names.split(','))
            for names in rsat_clusters_df[1].str.upper().values]
    assay_clusters = []
    motifs_not_found = []
    for assay in assays:
        ids = [i + 1 for i, motif_set in enumerate(sets) if assay in motif_set]     # rsat ids start from 1
        if not ids:
            ids = [MOTIF_NOT_FOUND_CLUSTER_ID]
            if assay not in motifs_not_found:
                motifs_not_found.append(assay)
        assay_clusters.append(ids)
    rsat_clusters_df = rsat_clusters_df.set_index(0)
    rsat_clusters_df.loc["cluster_-1"] = ",".join(motifs_not_found)
    return assay_clusters, rsat_clusters_df


def clusters_from_assay_ids(assay_clusters):
    """Cluster ids in the order the marks first reach them (the reference's dict,
    predict_by_cluster_rsat.py:135-142) and, per id, its marks in ascending order."""
    members = {}
    for f, ids in enumerate(assay_clusters):
        for cid in ids:
            members.setdefault(cid, []).append(f)
    return list(members), list(members.values())


def feature_clusters(path: str, n_keep: int):
    """Column ``cluster`` of all_feature_clusters.tsv -> (sorted labels, marks per label)."""
    labels = pd.read_csv(path, sep='\t', index_col=0)['cluster'].to_numpy()
    if len(labels) == 10 * n_keep:
        per_mark = labels.reshape(n_keep, 10)
        if (per_mark != per_mark[:, :1]).any():
            raise ValueError("feature clusters: the 10 coefficients of a mark carry different labels; "
                             "clusters here are sets of marks")
        labels = per_mark[:, 0]
    elif len(labels) != n_keep:
        raise ValueError(f"feature clusters: {len(labels)} rows for {n_keep} kept marks "
                         "(one per mark, or one per mark and coeff_idx)")
    ids = sorted(set(labels.tolist()))
    return ids, [np.nonzero(labels == c)[0].tolist() for c in ids]


def model_dirs(out_dir: str, model_files) -> list:
    """One model: the reference layout in out_dir.  More: ``<out_dir>/<model file stem>/``."""
    if len(model_files) == 1:
        return [out_dir]
    stems = [os.path.splitext(os.path.basename(f))[0] for f in model_files]
    if len(set(stems)) != len(stems):
        raise ValueError("model files of one run need distinct file stems")
    return [os.path.join(out_dir, s) for s in stems]


def run(args) -> list:
    rsat = args.rsat_clusters_tab is not None
    if rsat == (args.feature_clusters_df is not None):
        raise ValueError("give one of --rsat_clusters_tab and --feature_clusters_df")
    if rsat and not args.intersect_with_lambert:
        raise ValueError("--rsat_clusters_tab needs --intersect_with_lambert (the HGNC assay names)")
    model_files = [f.strip() for f in args.model_save_file]
    out_dirs = model_dirs(args.out_dir, model_files)
    for d in [args.out_dir] + out_dirs:
        os.makedirs(d, exist_ok=True)
    dev = _lib.device_of()
    beluga_features_df = predict.read_features_table(args.belugaFeatures)
    mask_args = predict.mask_arguments(args)
    # predict_by_cluster_rsat.py:68 prints the filter messages here; predict_by_cluster.py has no such call
    with contextlib.redirect_stdout(sys.stdout if rsat else io.StringIO()):
        keep_mask, hgnc_df = predict.get_keep_mask(beluga_features_df, *mask_args, return_hgnc_df=True)
    keep_idx = np.nonzero(keep_mask)[0].astype(np.int32)
    if rsat:
        hgnc_df = hgnc_df[keep_mask]
        assay_clusters, rsat_clusters_df = rsat_clusters(args.rsat_clusters_tab, hgnc_df["Assay"])
        cluster_ids, members = clusters_from_assay_ids(assay_clusters)
        contrib_columns = (hgnc_df['Assay'] + '/' + hgnc_df['Cell type']).to_numpy()
        ext = "tsv"
    else:
        cluster_ids, members = feature_clusters(args.feature_clusters_df, len(keep_idx))
        cluster_ids = list(range(len(cluster_ids)))
        contrib_columns = beluga_features_df['Assay type + assay + cell type'][keep_mask].to_numpy()
        ext = "csv"

    models = [GBLinear.load(f, base_score=args.base_score) for f in model_files]
    shifts = shift_order(int(args.maxshift))
    eff = predict.load_effects(args.snpEffectFilePattern, shifts, dev)
    rows = predict.Rows(args, dev)

    def batch_messages(in_batch):
        if rsat or in_batch:
            predict.get_keep_mask(beluga_features_df, *mask_args)
    ref, alt = predict.score_rows(args, models, eff, rows, keep_idx, shifts, batch_messages, dev)
    if not rsat:
        predict.get_keep_mask(beluga_features_df, *mask_args)          # predict_by_cluster.py:298 (messages)

    weights = np.stack([m.dump_weights() for m in models])
    prop = np.zeros((len(models), rows.n, len(keep_idx)))
    clu_prop = np.zeros((len(models), rows.n, len(members)))
    bs = int(args.batchSize)
    for lo in range(0, rows.n, bs):            # the reference's batches: device memory follows --batchSize
        hi = min(rows.n, lo + bs)
        sel = rows.ridx[lo:hi]
        res = variant_contributions(eff["ref"][:, sel], eff["alt"][:, sel], rows.dist[lo:hi], rows.strand_plus[lo:hi],
                                    shifts, keep_idx, weights, clusters=members, outputs=("prop", "clu_prop"))
        prop[:, lo:hi] = res.prop.cpu().numpy()
        clu_prop[:, lo:hi] = res.clu_prop.cpu().numpy()

    frames = []
    for m, out_dir in enumerate(out_dirs):
        df = predict.sed_frame(rows, ref[m], alt[m])
        df.to_csv(f'{out_dir}/sed.csv', header=True, sep='\t', index=False)
        predict.write_sorted(df, out_dir, ext)
        base = predict.with_proportion(df)
        for name, values, columns in (
                ("sed_sorted_by_proportion_with_contribs", prop[m], contrib_columns),
                ("cluster_contribs", clu_prop[m], [f'cluster_{idx}' for idx in cluster_ids])):
            table = pd.concat([base, pd.DataFrame(values, columns=columns)], axis=1)
            table = table.sort_values(by='SED_PROPORTION', axis=0, ascending=False).reset_index(drop=True)
            table.to_csv(f'{out_dir}/{name}.{ext}', header=True, sep='\t', index=False)
        if rsat:
            rsat_clusters_df.to_csv(f"{out_dir}/rsat_clusters.tsv", sep="\t", header=None)
        frames.append(df)
    return frames


def main(argv=None):
    args = build_parser().parse_args(argv)
    _lib.require_gpu("predict_by_cluster")
    return run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
