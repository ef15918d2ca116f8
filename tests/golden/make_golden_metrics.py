"""Writes tests/golden/metrics/values.json: what scipy, sklearn and numpy give for the seeded inputs of
tests/metrics_ref.py (``pair_case`` / ``stats_case``), so that the tests need none of them.

    python tests/golden/make_golden_metrics.py

Per pair case (n, ties): scipy's ``rankdata`` of pred and y, doubled (exact integers; as lists up to n = 4099,
as the SHA-256 of the little-endian int32 array above), ``spearmanr``, ``pearsonr`` and sklearn's ``r2_score``.
Per statistics case (B, F): ``np.mean(W, axis=0)`` and ``np.std(W, axis=0, ddof=1)``.  The inputs are
regenerated from their seeds by the tests.
"""
import hashlib
import json
import os
import sys

import numpy as np
import scipy
import sklearn
from scipy.stats import pearsonr, rankdata, spearmanr
from sklearn.metrics import r2_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from metrics_ref import PAIR_CASES, STATS_CASES, pair_case, stats_case  # noqa: E402

LIST_MAX = 4099


def doubled(x):
    r = 2.0 * rankdata(x, method="average")
    assert (r == np.round(r)).all()
    return r.astype("<i4")


def ranks_entry(x):
    r = doubled(x)
    return [int(v) for v in r] if r.shape[0] <= LIST_MAX else {"sha256": hashlib.sha256(r.tobytes()).hexdigest()}


def main():
    out = {"versions": {"numpy": np.__version__, "scipy": scipy.__version__, "sklearn": sklearn.__version__},
           "pairs": [], "stats": []}
    for n, ties in PAIR_CASES:
        pred, y = pair_case(n, ties)
        # the reference calls pearsonr(ytrue, ypred), r2_score(y_true=ytrue, y_pred=ypred), spearmanr(ytrue, ypred)
        out["pairs"].append({"n": n, "ties": ties, "rank2_pred": ranks_entry(pred), "rank2_y": ranks_entry(y),
                             "spearmanr": float(spearmanr(y, pred)[0]), "pearsonr": float(pearsonr(y, pred)[0]),
                             "r2_score": float(r2_score(y_true=y, y_pred=pred))})
    for B, F in STATS_CASES:
        W, _ = stats_case(B, F)
        out["stats"].append({"B": B, "F": F, "mean": [float(v) for v in np.mean(W, axis=0)],
                             "std_ddof1": [float(v) for v in np.std(W, axis=0, ddof=1)]})
    os.makedirs(os.path.join(HERE, "metrics"), exist_ok=True)
    with open(os.path.join(HERE, "metrics", "values.json"), "w") as f:
        json.dump(out, f)
        f.write("\n")


if __name__ == "__main__":
    main()
