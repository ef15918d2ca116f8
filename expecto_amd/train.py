"""Drop-in for the reference ``train.py`` / ``train_bootstrap.py`` CLIs: TSS features
(``Xreducedall*.npy``) and an expression table -> ExPecto gblinear models, trained on the GPU.

    python -m expecto_amd.train --expFile geneanno.exp.csv --targetIndex 1 \\
        --belugaFeatures features.tsv --inputFile Xreducedall.2002.npy --output_dir models

Same arguments and defaults as ``train.py:27-77``, the same row selection (``train.py:86-100``,
``:127-138``: train = every gene off chrX, chrY and chr8, test = chr8, both under the
``--filterStr`` filter and the finite-log filter), the same ``Cell type:`` / ``Training data
shape:`` / ``[i]\\teval-rmse:%f\\ttrain-rmse:%f`` / Spearman lines and the same ``.save`` /
``.dump`` file names (``train.py:156-159``).  ``xgb.train`` is replaced by
:func:`expecto_amd.xgblinear.train` (xgboost is not needed); ``--threads`` is accepted and
ignored (the single-thread update order is the definition).

Additions: ``--targetIndex`` takes several column indices or ``all`` (every column but the
first); targets with the same row selection are trained as one batch on one device copy of the
features.  ``--n_bootstrap K --seed S`` folds in ``train_bootstrap.py``: replicate k draws
``np.random.RandomState(S + k).choice(trainind, trainind.size, replace=True)`` (replicate 0 is
the draw of ``train_bootstrap.py --seed S``) and trains on the draw counts as row weights, not
on a gathered copy; its files carry ``.boot{k}`` ahead of the extension.  ``--l1`` is passed on
as ``alpha`` (the reference parses it and then trains with ``alpha: 0``; the default is 0).
``--holdout CHR [CHR ...]`` takes those chromosomes out of the training rows as well
(``train_susztak.py:117-120`` holds out chr7).  ``--metrics`` scores every model of a batch on the
device (:mod:`expecto_amd.metrics`: Pearson r, Spearman r and R2 on its unweighted train rows and
on its chr8 rows, labels in float64) and writes ``<output_dir>/metrics/metrics.h5`` (the datasets
of ``train_susztak.py:177-181`` plus ``spearmanr_trains`` / ``spearmanr_valids``, in model order)
and ``metrics.tsv``.  Both are off by default, and then nothing changes.

``--cv K`` chooses the penalties and the number of rounds per target by K-fold cross-validation
(:func:`expecto_amd.xgblinear.cv`) before it trains: the folds are whole chromosomes of the
training rows (``chromosome_folds``), the grid is ``--l2-grid`` x ``--l1-grid`` (each defaults to
the single ``--l2`` / ``--l1``) from most to least regularised, every round up to ``--num_round``
is a candidate, and ``--cv-rule`` picks the least mean held-out rmse (``min``) or the most
regularised grid point within one standard error of it (``1se``).  ``cv.tsv`` (one row per target,
l2, l1 and round: score, se and the held-out rmse of every fold), ``cv_best.tsv`` (one row per
target: l2, l1, num_round, score, se) and ``cv_folds.tsv`` (chromosome, fold, rows) go to
``--output_dir``.  Each target is then trained on all training rows at its choice, and its lines,
files and metrics are those of a plain run with ``--l2``, ``--l1`` and ``--num_round`` set to it;
``--cv-only`` stops after the tables.  ``--cv`` with ``--n_bootstrap`` is refused.

Left out: the scatter plots (``train.py:161-184``), ``--kidney_genes_only`` and
``--match_with_basenji2`` (the latter reads a hard-coded path of its author's machine).
``--annoFile`` is honoured (the reference parses it and reads ``./resources/geneanno.csv``,
its default, regardless).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from .predict import NFEAT, get_keep_mask
from .xgblinear import ColMatrix, cv, predict_cols, train


def build_parser(cv: bool = False):
    """The arguments of the reference CLIs and the additions above; ``cv=True`` (what ``main`` uses) adds
    the cross-validation flags.  ``run`` treats a namespace without them as cross-validation off."""
    p = argparse.ArgumentParser(description='Process some integers.')
    p.add_argument('--targetIndex', action="store", dest="targetIndex", nargs='+', required=True,
                   help="column(s) of expFile to train on, or 'all'")
    add_reference_arguments(p)
    p.add_argument('--n_bootstrap', type=int, default=0, help="bootstrap replicates per target (0: none)")
    p.add_argument('--seed', action="store", dest="seed", type=int, default=0)
    p.add_argument('--holdout', nargs='+', default=[], metavar='CHR',
                   help="chromosomes taken out of the training rows (train_susztak.py holds out chr7)")
    p.add_argument('--metrics', action='store_true', default=False,
                   help="score every model on its train and test rows; write metrics/metrics.h5 and metrics.tsv")
    if cv:
        add_cv_arguments(p)
    return p


def add_cv_arguments(p):
    """The cross-validation flags (module docstring), all off by default."""
    p.add_argument('--cv', type=int, default=0, metavar='K',
                   help="choose l2, l1 and the number of rounds per target by K-fold cross-validation over "
                        "whole chromosomes (0: off)")
    p.add_argument('--l2-grid', dest='l2_grid', type=float, nargs='+', default=None, help="default: --l2 alone")
    p.add_argument('--l1-grid', dest='l1_grid', type=float, nargs='+', default=None, help="default: --l1 alone")
    p.add_argument('--cv-rule', dest='cv_rule', choices=('min', '1se'), default='min')
    p.add_argument('--cv-only', dest='cv_only', action='store_true', default=False,
                   help="write the cross-validation tables and train nothing further")


def add_reference_arguments(p):
    """The arguments train.py:27-77 and train_susztak.py:28-69 share."""
    p.add_argument('--expFile', action="store", dest="expFile")
    p.add_argument('--belugaFeatures', action="store", dest="belugaFeatures", help="tsv file denoting Beluga features")
    p.add_argument('--inputFile', action="store", dest="inputFile", default='./resources/Xreducedall.2002.npy')
    p.add_argument('--annoFile', action="store", dest="annoFile", default='./resources/geneanno.csv')
    p.add_argument('--evalFile', action="store", dest="evalFile", default='',
                   help='specify to save holdout set predictions')
    p.add_argument('--filterStr', action="store", dest="filterStr", type=str, default="all")
    p.add_argument('--pseudocount', action="store", dest="pseudocount", type=float, default=0.0001)
    p.add_argument('--num_round', action="store", dest="num_round", type=int, default=100)
    p.add_argument('--l2', action="store", dest="l2", type=float, default=100)
    p.add_argument('--l1', action="store", dest="l1", type=float, default=0)
    p.add_argument('--eta', action="store", dest="eta", type=float, default=0.01)
    p.add_argument('--base_score', action="store", dest="base_score", type=float, default=2)
    p.add_argument('--threads', action="store", dest="threads", type=int, default=16, help="accepted and ignored")
    p.add_argument('--no_tf_features', action='store_true', dest='no_tf_features', default=False)
    p.add_argument('--no_dnase_features', action='store_true', dest='no_dnase_features', default=False)
    p.add_argument('--no_histone_features', action='store_true', dest='no_histone_features', default=False)
    p.add_argument('--intersect_with_lambert', action='store_true', dest='intersect_with_lambert', default=False)
    p.add_argument('--no_pol2', action='store_true', dest='no_pol2', default=False)
    p.add_argument('--output_dir', type=str, default='temp_expecto_model')


def gene_filter(geneanno: pd.DataFrame, filter_str: str) -> np.ndarray:
    """train.py:86-93."""
    if filter_str == 'pc':
        return np.asarray(geneanno.iloc[:, -1] == 'protein_coding')
    if filter_str == 'lincRNA':
        return np.asarray(geneanno.iloc[:, -1] == 'lincRNA')
    if filter_str == 'all':
        return np.asarray(geneanno.iloc[:, -1] != 'rRNA')
    raise ValueError('filterStr has to be one of all, pc, and lincRNA')


def select_rows(geneanno: pd.DataFrame, expr: pd.Series, filter_str: str, pseudocount: float, holdout=()):
    """Boolean (train, test) masks over the genes for one expression column (train.py:86-100,
    :127-132); ``holdout`` chromosomes leave the training rows as well (train_susztak.py:117-120)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        filt = gene_filter(geneanno, filter_str) * np.isfinite(np.asarray(np.log(expr + pseudocount)))
    trainind = np.asarray(geneanno['seqnames'] != 'chrX') * np.asarray(
        geneanno['seqnames'] != 'chrY') * np.asarray(geneanno['seqnames'] != 'chr8')
    for c in holdout:
        trainind = trainind * np.asarray(geneanno['seqnames'] != c)
    testind = np.asarray(geneanno['seqnames'] == 'chr8')
    return np.asarray(trainind * filt, dtype=bool), np.asarray(testind * filt, dtype=bool)


def bootstrap_weights(train_mask: np.ndarray, seed: int) -> np.ndarray:
    """Draw counts per gene of train_bootstrap.py:88-90 under ``np.random.seed(seed)``: training on
    rows ``choice(trainind, size, replace=True)`` is training on every row with its count as weight."""
    trainind = np.where(train_mask)[0]
    draw = np.random.RandomState(seed).choice(trainind, size=trainind.shape[0], replace=True)
    return np.bincount(draw, minlength=train_mask.shape[0])


def chromosome_folds(seqnames, K: int):
    """K folds of whole chromosomes over rows named by ``seqnames``: the chromosomes by row count
    descending, then name, each to the fold with the fewest rows so far (the lowest index on a tie).
    Returns (fold int64 per row, [(chromosome, fold, rows)] in that order)."""
    seqnames = np.asarray(seqnames, dtype=str)
    names, counts = np.unique(seqnames, return_counts=True)
    if K < 2:
        raise ValueError("--cv needs at least 2 folds")
    if len(names) < K:
        raise ValueError(f"--cv {K}: the training rows span only {len(names)} chromosomes")
    order = sorted(zip(names.tolist(), counts.tolist()), key=lambda c: (-c[1], c[0]))
    size, fold_of = [0] * K, {}
    for name, rows in order:
        k = min(range(K), key=lambda i: (size[i], i))
        fold_of[name] = k
        size[k] += rows
    fold = np.array([fold_of[s] for s in seqnames.tolist()], dtype=np.int64)
    return fold, [(name, fold_of[name], rows) for name, rows in order]


def penalty_grid(l2s, l1s) -> list:
    """The product of the two lists as (l2, l1) pairs, by descending l2, then descending l1: from the
    most to the least regularised, the order ``--cv-rule 1se`` prefers."""
    return sorted(((float(a), float(b)) for a in l2s for b in l1s), key=lambda p: (-p[0], -p[1]))


def check_cv_args(args) -> None:
    """Refuse flag combinations that cross-validation does not cover, before any file is read."""
    K = int(getattr(args, 'cv', 0) or 0)
    if K == 0:
        for flag in ('l2_grid', 'l1_grid'):
            if getattr(args, flag, None) is not None:
                raise ValueError(f"--{flag.replace('_', '-')} needs --cv")
        if getattr(args, 'cv_only', False) or getattr(args, 'cv_rule', 'min') != 'min':
            raise ValueError("--cv-rule and --cv-only need --cv")
        return
    if K < 2:
        raise ValueError("--cv needs at least 2 folds")
    if args.n_bootstrap > 0:
        raise ValueError("--cv with --n_bootstrap is not supported: cross-validate first, then bootstrap at the "
                         "chosen --l2, --l1 and --num_round")
    if args.num_round < 1:
        raise ValueError("--cv needs --num_round >= 1")


def write_cv_tables(output_dir: str, K: int, rows: list, folds: list) -> None:
    """cv.tsv, cv_best.tsv and cv_folds.tsv.  rows: (target name, CVResult, index of the target in
    it) per target; folds: (target names, chromosome table) per group of targets sharing rows."""
    with open(f'{output_dir}/cv.tsv', 'w') as f, open(f'{output_dir}/cv_best.tsv', 'w') as fb:
        f.write('\t'.join(['target', 'l2', 'l1', 'round', 'score', 'se'] + [f'fold{k}' for k in range(K)]) + '\n')
        fb.write('\t'.join(['target', 'l2', 'l1', 'num_round', 'score', 'se']) + '\n')
        for name, res, t in rows:
            for g, (l2, l1) in enumerate(res.grid):
                for r in range(res.score.shape[2]):
                    f.write('\t'.join([str(name), repr(float(l2)), repr(float(l1)), str(r + 1)] + [
                        '%.17g' % v for v in (res.score[t, g, r], res.se[t, g, r], *res.heldout[t, g, :, r])]) + '\n')
            g, r = int(res.best_g[t]), int(res.best_round[t])
            fb.write('\t'.join([str(name), repr(float(res.grid[g, 0])), repr(float(res.grid[g, 1])), str(r),
                                '%.17g' % res.score[t, g, r - 1], '%.17g' % res.se[t, g, r - 1]]) + '\n')
    with open(f'{output_dir}/cv_folds.tsv', 'w') as f:
        f.write('chromosome\tfold\trows\n')
        for names, table in folds:
            if len(folds) > 1:                         # targets whose finite-log filters differ have their own rows
                f.write('# targets: ' + ','.join(str(n) for n in names) + '\n')
            for chrom, k, n in table:
                f.write(f'{chrom}\t{k}\t{n}\n')


def target_indices(spec, ncols: int) -> list:
    if len(spec) == 1 and spec[0] == 'all':
        return list(range(1, ncols))
    return [int(s) for s in spec]


def spearman_line(ypred, ytrue) -> str:
    try:
        from scipy.stats import spearmanr
        return str(spearmanr(ypred, ytrue))
    except ImportError:
        rho = np.corrcoef(pd.Series(ypred).rank(), pd.Series(ytrue).rank())[0, 1]
        return f"SignificanceResult(statistic={rho}, pvalue=nan)"


METRIC_NAMES = ('pearsonr_trains', 'pearsonr_valids', 'spearmanr_trains', 'spearmanr_valids', 'r2_trains',
                'r2_valids')


def write_metrics(output_dir: str, results: list) -> None:
    """``<output_dir>/metrics/metrics.h5`` with the four datasets of train_susztak.py:177-181 and the two
    Spearman ones, float64 in model order, and ``metrics.tsv`` with the same figures per model."""
    from . import h5

    metrics_dir = f'{output_dir}/metrics'
    os.makedirs(metrics_dir, exist_ok=True)
    cols = {k: np.array([r["metrics"][k] for r in results], dtype=np.float64) for k in METRIC_NAMES}
    h5.write(f'{metrics_dir}/metrics.h5', cols)
    with open(f'{metrics_dir}/metrics.tsv', 'w') as f:
        f.write('\t'.join(('name', 'boot') + METRIC_NAMES) + '\n')
        for m, r in enumerate(results):
            f.write('\t'.join([str(r["name"]), '' if r["boot"] is None else str(r["boot"])] +
                              ['%.17g' % cols[k][m] for k in METRIC_NAMES]) + '\n')


def run(args, model_dir=None) -> list:
    """Train every requested model; returns one dict per model (name, boot, model, history,
    save, dump; with ``--metrics`` also metrics) in the order their lines were printed.  The model
    files go to ``model_dir`` (default: ``args.output_dir``)."""
    holdout, want_metrics = getattr(args, 'holdout', None) or [], bool(getattr(args, 'metrics', False))
    check_cv_args(args)
    cv_k = int(getattr(args, 'cv', 0) or 0)
    cv_rows, cv_fold_tables = [], []
    model_dir = args.output_dir if model_dir is None else model_dir
    os.makedirs(args.output_dir, exist_ok=True)
    os.makedirs(model_dir, exist_ok=True)
    X = np.load(args.inputFile)
    geneanno = pd.read_csv(args.annoFile)
    geneexp = pd.read_csv(args.expFile)
    targets = target_indices(args.targetIndex, geneexp.shape[1])

    beluga_features_df = pd.read_csv(args.belugaFeatures, sep='\t', index_col=0)
    beluga_features_df['Assay type + assay + cell type'] = (beluga_features_df['Assay type'] + '/' +
                                                           beluga_features_df['Assay'] + '/' +
                                                           beluga_features_df['Cell type'])
    keep_mask = get_keep_mask(beluga_features_df, args.no_tf_features, args.no_dnase_features,
                              args.no_histone_features, args.intersect_with_lambert, args.no_pol2)
    keep_indices = np.nonzero(keep_mask)[0]
    num_genes = X.shape[0]
    X = X.reshape(num_genes, 10, NFEAT)[:, :, keep_indices].reshape(num_genes, -1)
    print(f'Training data shape: {X.shape}')

    # targets with the same row selection share one device copy of the features and one batch
    groups = {}
    for ti in targets:
        tr, te = select_rows(geneanno, geneexp.iloc[:, ti], args.filterStr, args.pseudocount, holdout)
        groups.setdefault((tr.tobytes(), te.tobytes()), (tr, te, []))[2].append(ti)

    results = []
    for tr, te, tis in groups.values():
        Xtr, Xte = ColMatrix(X[tr]), ColMatrix(X[te])
        jobs = []                                      # (target, replicate or None, y_train, weight, y_test)
        for ti in tis:
            ylog = np.asarray(np.log(geneexp.iloc[:, ti] + args.pseudocount))
            reps = [None] if args.n_bootstrap <= 0 else list(range(args.n_bootstrap))
            for k in reps:
                wgt = np.ones(int(tr.sum())) if k is None else bootstrap_weights(tr, args.seed + k)[tr]
                jobs.append((ti, k, ylog[tr], wgt, ylog[te]))
        ytr = np.stack([j[2] for j in jobs])
        wtr = np.stack([j[3] for j in jobs]) if args.n_bootstrap > 0 else None
        yte = np.stack([j[4] for j in jobs])
        if cv_k:
            grid = penalty_grid(args.l2_grid or [args.l2], args.l1_grid or [args.l1])
            fold, table = chromosome_folds(np.asarray(geneanno['seqnames'])[tr], cv_k)
            chosen = cv(Xtr, ytr, fold, grid, num_round=args.num_round, eta=args.eta, base_score=args.base_score,
                        rule=args.cv_rule)
            cv_rows += [(geneexp.columns[ti], chosen, t) for t, ti in enumerate(tis)]
            cv_fold_tables.append(([geneexp.columns[ti] for ti in tis], table))
            if args.cv_only:
                continue
            models, history = chosen.refit(Xtr, ytr, evals=[(Xte, yte)], with_history=True)
            settings = [(float(chosen.grid[g, 0]), int(r)) for g, r in zip(chosen.best_g, chosen.best_round)]
        else:
            models, history = train(Xtr, ytr, wtr, num_round=args.num_round, eta=args.eta, lambda_=args.l2,
                                    alpha=args.l1, base_score=args.base_score, evals=[(Xte, yte)])
            settings = [(args.l2, args.num_round)] * len(jobs)
        ypred_dev = predict_cols(Xte, models)
        ypred = ypred_dev.cpu().numpy()
        if want_metrics:
            # labels in float64 as the reference hands them to scipy; train-set figures are unweighted
            from .metrics import model_metrics
            scores = np.concatenate([model_metrics(predict_cols(Xtr, models), ytr), model_metrics(ypred_dev, yte)], 1)
        for m, (ti, k, _, _, ytrue) in enumerate(jobs):
            name = geneexp.columns[ti]
            print(f"Cell type: {name}" + ("" if k is None else f" (bootstrap {k})"))
            l2, num_round = settings[m]
            for r in range(num_round):
                print("[%d]\teval-rmse:%f\ttrain-rmse:%f" % (r, history[m][r, 1], history[m][r, 0]))
            print(spearman_line(ypred[m], ytrue))
            tag = "" if k is None else f".boot{k}"
            if args.evalFile != '':
                path = args.evalFile if len(jobs) == 1 and len(groups) == 1 else f"{args.evalFile}.{name}{tag}"
                pd.DataFrame({'pred': ypred[m], 'target': ytrue}).to_csv(path)
            stem = (f'{model_dir}/expecto_{args.filterStr}.pseudocount{args.pseudocount}.lambda{l2}'
                    f'.round{num_round}.basescore{args.base_score}.{name}{tag}')
            models[m].save_legacy(stem + '.save')
            models[m].save_dump(stem + '.dump')
            results.append({"name": name, "boot": k, "model": models[m], "history": history[m],
                            "save": stem + '.save', "dump": stem + '.dump'})
            if want_metrics:
                pt, st, rt, pv, sv, rv = (float(v) for v in scores[m])
                results[-1]["metrics"] = {'pearsonr_trains': pt, 'pearsonr_valids': pv, 'spearmanr_trains': st,
                                          'spearmanr_valids': sv, 'r2_trains': rt, 'r2_valids': rv}
    if cv_k:
        write_cv_tables(args.output_dir, cv_k, cv_rows, cv_fold_tables)
    if want_metrics and not (cv_k and args.cv_only):
        write_metrics(args.output_dir, results)
    return results


def main(argv=None):
    from . import _lib

    args = build_parser(cv=True).parse_args(argv)
    _lib.require_gpu("train")
    return run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
