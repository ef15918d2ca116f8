"""Scores of trained models and statistics of a bootstrap batch, on the GPU (csrc/metrics.hip).

The reference judges its models on the host, one at a time: ``scipy.stats.pearsonr`` / ``spearmanr`` and
``sklearn.metrics.r2_score`` in the ``plot_preds`` of ``train.py``, ``train_bootstrap.py``,
``train_susztak.py`` and the ``geuvadis_predict_consensus*.py`` scripts, and ``np.std(ddof=1)`` over the
bootstrap models in ``plot_bootstrapped_coefficients.py:52-76``.  Here a batch of models is scored where its
predictions already lie:

* ``rank2(x)``: doubled average ranks, ``2 * rankdata(x, 'average')`` as exact integers, by counting;
* ``model_metrics(pred, y)``: ``(pearson, spearman, r2)`` per model; Spearman from exact integer sums of the
  doubled ranks, Pearson and R2 in float64 in a stated order (include/expecto_hip.h);
* ``bootstrap_coef_stats(boot_weights, main_weights)``: per-coefficient mean, standard error, z-score and
  coefficient of variation.

There is no CPU path.  p-values are not computed (``train.spearman_line`` keeps printing scipy's).
"""
from __future__ import annotations

import numpy as np

MAX_ROWS = 32768          # EXPECTO_METRICS_MAX_ROWS
RANK_TILE = 256           # elements of a row one workgroup of expecto_rank2_* owns
RANK_LDS_TILE = 2048      # values of the row it holds in LDS at a time
MAX_BOOT = 4096


def _to_device(a, dtype=None):
    import torch

    from . import _lib
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if not t.is_cuda:
        t = t.to(_lib.device_of())
    return t if dtype is None or t.dtype == dtype else t.to(dtype)


def rank2(x):
    """Doubled average ranks of every row of ``x`` (``[n]`` or ``[P, n]``, float32 or float64, host or
    device): an int32 device tensor of the same shape with ``2 * #{x_j < x_i} + #{x_j == x_i} + 1``."""
    import torch

    from . import _lib

    t = _to_device(x)
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"rank2: float32 or float64 values, not {t.dtype}")
    if t.dim() not in (1, 2):
        raise ValueError("rank2: x must be [n] or [P, n]")
    rows = t if t.dim() == 2 else t.unsqueeze(0)
    if rows.shape[1] > 1 and rows.stride(1) != 1:
        rows = rows.contiguous()
    P, n = int(rows.shape[0]), int(rows.shape[1])
    if n > MAX_ROWS:
        raise ValueError(f"rank2: n = {n} exceeds {MAX_ROWS}")
    out = torch.empty(P, n, dtype=torch.int32, device=rows.device)
    name = "expecto_rank2_f32" if t.dtype == torch.float32 else "expecto_rank2_f64"
    for p0 in range(0, P, 65535):                                   # the grid's y limit
        part = rows[p0:p0 + 65535]
        _lib.call(name, _lib.dptr(part), part.stride(0) if part.shape[0] > 1 else 0, n, int(part.shape[0]),
                  _lib.dptr(out[p0:]), what="rank2")
    return out if t.dim() == 2 else out[0]


def model_metrics(pred, y) -> np.ndarray:
    """``[P, 3]`` float64 ``(pearson, spearman, r2)`` of predictions ``pred`` (``[P, n]`` float32, host or
    device) against labels ``y`` (float64, ``[n]`` shared by every model or ``[P, n]``).  The ranks of a
    shared ``y`` are computed once.  ``ValueError`` for n < 2 or n > 32768."""
    import torch

    from . import _lib

    p = _to_device(pred)
    if p.dim() != 2 or p.dtype != torch.float32:
        raise ValueError("model_metrics: pred must be float32 [P, n]")
    p = p if p.stride(1) == 1 else p.contiguous()
    P, n = int(p.shape[0]), int(p.shape[1])
    if n < 2 or n > MAX_ROWS:
        raise ValueError(f"model_metrics: n = {n} outside [2, {MAX_ROWS}]")
    t = _to_device(y, torch.float64).contiguous()
    if t.shape not in ((n,), (P, n)):
        raise ValueError(f"model_metrics: y must be [n] or [P, n] with P = {P}, n = {n}")
    shared = t.dim() == 1
    out = torch.empty(P, 3, dtype=torch.float64, device=p.device)
    if P:
        ra, rb = rank2(p), rank2(t)
        _lib.call("expecto_model_metrics", _lib.dptr(p), p.stride(0), _lib.dptr(t), 0 if shared else n, _lib.dptr(ra),
                  _lib.dptr(rb), n, P, _lib.dptr(out), what="model_metrics")
    return out.cpu().numpy()


def bootstrap_coef_stats(boot_weights, main_weights) -> dict:
    """Per-coefficient statistics of ``boot_weights`` (``[B, F]`` float64, one row per bootstrap model)
    and the main model's ``main_weights`` (``[F]``): ``{"mean", "se", "z", "cv"}``, float64 ``[F]`` host
    arrays (``np.mean(axis=0)``, ``np.std(axis=0, ddof=1)``, ``main / se``, ``se / |mean|``)."""
    import torch

    from . import _lib

    W = _to_device(boot_weights, torch.float64)
    w = _to_device(main_weights, torch.float64).contiguous()
    if W.dim() != 2 or (W.shape[1] > 1 and W.stride(1) != 1):
        W = W.contiguous()
    if W.dim() != 2 or w.shape != (W.shape[1],):
        raise ValueError("bootstrap_coef_stats: boot_weights [B, F] and main_weights [F]")
    B, F = int(W.shape[0]), int(W.shape[1])
    if B < 2 or B > MAX_BOOT:
        raise ValueError(f"bootstrap_coef_stats: B = {B} outside [2, {MAX_BOOT}]")
    out = torch.empty(4, F, dtype=torch.float64, device=W.device)
    _lib.call("expecto_bootstrap_coef_stats", _lib.dptr(W), max(W.stride(0), F), B, F, _lib.dptr(w), _lib.dptr(out[0]),
              _lib.dptr(out[1]), _lib.dptr(out[2]), _lib.dptr(out[3]), what="bootstrap_coef_stats")
    h = out.cpu().numpy()
    return {"mean": h[0], "se": h[1], "z": h[2], "cv": h[3]}
