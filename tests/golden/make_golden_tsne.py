"""Golden outputs of scikit-learn's exact t-SNE.

Run from the repo root on a CPU machine (needs scikit-learn 1.7.2; it is not read at test time):
    python tests/golden/make_golden_tsne.py

Writes tests/golden/tsne/sklearn.npz: for every ``tsne_ref.CASES`` entry ``<case>_X`` and ``<case>_Y0``
(the recipe inputs of ``tsne_ref.case_inputs``), ``<case>_params`` = [perplexity, early_exaggeration,
learning_rate, max_iter], and ``<case>_Y``, ``<case>_kl``, ``<case>_n_iter`` =
``TSNE(method='exact', init=Y0, **params)``'s ``fit_transform(X)``, ``kl_divergence_`` and ``n_iter_``.
The inputs have small-integer coordinates: their squared distances are exact in float32, so the cast
inside sklearn's ``_joint_probabilities`` loses nothing.
"""
from __future__ import annotations

import os
import sys

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(GOLD))
import tsne_ref  # noqa: E402

DST = os.path.join(GOLD, "tsne")


def sklearn_cases():
    from sklearn.manifold import TSNE
    out = {}
    for name in tsne_ref.CASES:
        X, Y0, kw = tsne_ref.case_inputs(name)
        ts = TSNE(n_components=2, method="exact", init=Y0.copy(), **kw)
        out[name + "_X"], out[name + "_Y0"] = X, Y0
        out[name + "_params"] = np.array([kw["perplexity"], kw["early_exaggeration"], kw["learning_rate"],
                                          kw["max_iter"]], np.float64)
        out[name + "_Y"] = ts.fit_transform(X.copy()).astype(np.float64)
        out[name + "_kl"] = np.float64(ts.kl_divergence_)
        out[name + "_n_iter"] = np.int32(ts.n_iter_)
    return out


def main():
    os.makedirs(DST, exist_ok=True)
    np.savez_compressed(os.path.join(DST, "sklearn.npz"), **sklearn_cases())
    print("t-SNE golden outputs written to", DST)


if __name__ == "__main__":
    main()
