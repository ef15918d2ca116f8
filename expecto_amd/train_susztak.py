"""Drop-in for the reference ``train_susztak.py``: one gblinear model per column of an expression
table, chr7 held out, chr8 the validation set, and the models' scores in ``metrics/metrics.h5``.

    python -m expecto_amd.train_susztak --expFile susztak.exp.csv --belugaFeatures features.tsv \\
        --inputFile Xreducedall.2002.npy --output_dir out

Same arguments and defaults as ``train_susztak.py:28-69``.  It is ``expecto_amd.train`` with
``--targetIndex all --holdout chr7 --metrics``: every column that shares a row selection trains as
one batch on the GPU, and the batch is scored there.  The models go to ``<output_dir>/models`` under
the reference's file names (``train_susztak.py:140-143``); ``<output_dir>/metrics/metrics.h5`` holds
``pearsonr_trains``, ``pearsonr_valids``, ``r2_trains`` and ``r2_valids`` (``:177-181``, what
``plot_susztak.py`` reads) plus ``spearmanr_trains`` / ``spearmanr_valids``, and ``metrics.tsv`` beside
it names the models.

Differences.  The reference re-slices ``Xreducedall`` by the ablation mask inside its per-column loop
(``:104-112``), so with any ablation flag its second column fails on the reshape; the features are
sliced once here.  ``--annoFile`` is honoured (the reference parses it and reads
``./resources/geneanno.csv``), ``--l1`` is passed on as ``alpha`` (the reference trains with 0; so does
the default), ``--evalFile`` and ``--threads`` are accepted and ignored as in the reference, and the
scatter plots (``:146-172``) are left out.
"""
from __future__ import annotations

import argparse
import sys

from . import train


def build_parser():
    p = argparse.ArgumentParser(description='Process some integers.')
    train.add_reference_arguments(p)
    return p


def run(args) -> list:
    full = argparse.Namespace(**vars(args))
    full.targetIndex, full.n_bootstrap, full.seed = ['all'], 0, 0
    full.holdout, full.metrics, full.evalFile = ['chr7'], True, ''
    return train.run(full, model_dir=f'{args.output_dir}/models')


def main(argv=None):
    from . import _lib

    args = build_parser().parse_args(argv)
    _lib.require_gpu("train_susztak")
    return run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
