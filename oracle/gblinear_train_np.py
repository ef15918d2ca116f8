"""CPU restatement of the gblinear training kernels, with the device's order of summation --
TEST INFRASTRUCTURE (oracle) ONLY.  numpy alone.

The steps are DESIGN.md "Training gblinear models": float32 state, every float32 product and
sum rounded on its own, the sums over rows in double.  tests/gblinear_ref.py states the same
steps with numpy's sum; here the double sums run through the tree of ``csrc/train.hip``, so the
results can be held to the kernels bit for bit.

The tree (``tree_sum``).  A workgroup has 1,024 lanes.  Lane ``t`` starts at +0.0 and adds the
terms of rows ``t, t + 1024, t + 2048, ...`` in that order (train.hip:113-129 ``cd_step``,
:187-204 the gradient step, :282-288 the rmse loop).  A row past ``n`` adds a zero of either
sign, which leaves a sum that started at +0.0 as it is, so it is left out here.  The 1,024 lane
sums are then combined by a balanced pairwise tree in natural order: neighbours, neighbouring
pairs, ... for ten levels.  That is what ``wave_sum`` (train.hip:38-50) and ``block_sum``
(train.hip:59-74) compute: every butterfly step adds the same two numbers on both partners and
float addition is commutative, so quad_perm [1,0,3,2] is level 1, quad_perm [2,3,0,1] level 2,
row_half_mirror (the other quad of a half row: all four lanes of a quad already agree) level 3,
row_mirror level 4, the shuffles over 16 and 32 lanes levels 5 and 6, and the 16 wave partials,
taken by lane ``l & 15`` and summed by the same row butterfly (train.hip:73), levels 7 to 10.

``delta`` uses fmax / fmin like the kernel (train.hip:77-82); they differ from xgboost's
std::max / std::min only where an operand is NaN.

A batch axis runs B independent models at once: y, h ``[B, n]``, w ``[B, F + 1]`` with the bias
last (the device layout), sh ``[B, F]``; X ``[n, F]`` is shared.
"""
from __future__ import annotations

import numpy as np

LANES = 1024
_f32 = np.float32


def tree_sum(v) -> np.ndarray:
    """Sum over the last axis of float64 ``v [..., n]`` in the device's order."""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    slots = max(1, -(-n // LANES))
    pad = np.zeros(v.shape[:-1] + (slots * LANES,))
    pad[..., :n] = v
    lane = np.zeros(v.shape[:-1] + (LANES,))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(slots):
            lane = lane + pad[..., k * LANES:(k + 1) * LANES]
        while lane.shape[-1] > 1:
            lane = lane[..., 0::2] + lane[..., 1::2]
    return lane[..., 0]


def delta(sg, sh, w, lam, alpha):
    """CoordinateDelta in double, element-wise over the batch."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = w - (sg + lam * w) / (sh + lam)
        pos = np.fmax(-(sg + lam * w + alpha) / (sh + lam), -w)
        neg = np.fmin(-(sg + lam * w - alpha) / (sh + lam), -w)
    return np.where(sh < 1e-5, 0.0, np.where(t >= 0, pos, neg))


def predict_cols(X, w, base) -> np.ndarray:
    """Rule 1: p = (b + base) + x_0 w_0 + x_1 w_1 + ... in column order -> float32 [B, n]."""
    X = np.asarray(X, _f32)
    w = np.atleast_2d(np.asarray(w, _f32))
    n, F = X.shape
    assert w.shape[1] == F + 1
    p = np.repeat((w[:, F] + _f32(base))[:, None], n, axis=1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(F):
            p = p + X[None, :, j] * w[:, j:j + 1]
    return p


def train_round(X, y, h, w, sh, first, eta, lam, alpha, lam_bias, base):
    """One boosting round.  Returns (w, sh, pred): the new weights, the hessian sums (computed if
    ``first``, else the ones given) and the prediction the round started from."""
    X = np.asarray(X, _f32)
    n, F = X.shape
    w = np.atleast_2d(np.asarray(w, _f32)).copy()
    B = w.shape[0]
    y = np.broadcast_to(np.atleast_2d(np.asarray(y, _f32)), (B, n))
    h = np.ones((B, n), _f32) if h is None else np.broadcast_to(np.atleast_2d(np.asarray(h, _f32)), (B, n))
    sh = np.zeros((B, F)) if first else np.atleast_2d(np.asarray(sh, np.float64)).copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        pred = predict_cols(X, w, base)
        g = (pred - y) * h
        b = w[:, F]
        sg = tree_sum(g.astype(np.float64))
        shh = tree_sum(h.astype(np.float64))
        db = (eta * (-(sg + lam_bias * b.astype(np.float64)) / (shh + lam_bias))).astype(_f32)
        g = g + h * db[:, None]
        for j in range(F):
            x = X[None, :, j]
            hx = h * x
            sgj = tree_sum((g * x).astype(np.float64))
            if first:
                sh[:, j] = tree_sum((hx * x).astype(np.float64))
            dw = (eta * delta(sgj, sh[:, j], w[:, j].astype(np.float64), lam, alpha)).astype(_f32)
            w[:, j] = w[:, j] + dw
            g = g + hx * dw[:, None]
        w[:, F] = b + db
    return w, sh, pred


def rmse(pred, y, h) -> np.ndarray:
    """xgboost's weighted rmse: the square and its product with h in float32, the two sums
    through the tree, sqrt(a / b) in double -> float64 [B]."""
    pred = np.atleast_2d(np.asarray(pred, _f32))
    B, n = pred.shape
    y = np.broadcast_to(np.atleast_2d(np.asarray(y, _f32)), (B, n))
    h = np.ones((B, n), _f32) if h is None else np.broadcast_to(np.atleast_2d(np.asarray(h, _f32)), (B, n))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        d = y - pred
        sq = d * d
        a = tree_sum((sq * h).astype(np.float64))
        b = tree_sum(h.astype(np.float64))
        return np.sqrt(a / b)
