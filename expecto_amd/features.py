"""Spatial-feature reductions on the device (HBM-bound kernels of reduce.hip).

* ``tss_pos_weights`` + ``tss_reduce``: ``compute_expecto_features.py:88-124`` --
  ``F[g, k*2002+f] = sum_s W[k,s] * 0.5*(fwd[g,s,f] + rc[g,s,f])`` in float64.
* ``fwd_rc_average``: ``predict.py:186-190`` ``(x[:N] + x[N:]) / 2``.
* ``variant_features``: ``predict.py:87-136`` -- exp(-c*floor(|d|/200)) weights per shift,
  split by upstream/downstream, summed over shifts into ``[n, 10*2002]`` float64.
* ``variant_contributions``: ``predict_by_cluster_rsat.py:105-144`` -- the expression effect
  split by mark and by mark cluster, for any number of models in one pass over the effects.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib

DECAY = (0.01, 0.02, 0.05, 0.1, 0.2)
TSS_SHIFTS = tuple(range(-20000, 20000, 200))     # compute_expecto_features.py:88


def tss_pos_weights(shifts=TSS_SHIFTS) -> np.ndarray:
    """10 x S float64 (compute_expecto_features.py:91-101)."""
    s = np.asarray(shifts)
    rows = [np.exp(-c * np.abs(s) / 200) * (s <= 0) for c in DECAY]
    rows += [np.exp(-c * np.abs(s) / 200) * (s >= 0) for c in DECAY]
    return np.vstack(rows)


def tss_reduce(fwd: torch.Tensor, rc: torch.Tensor, weights: torch.Tensor, out: torch.Tensor | None = None):
    """fwd, rc: [G, S, F] fp32 (device); weights [10, S] fp64 (device) -> [G, 10*F] fp64."""
    G, S, F = fwd.shape
    if rc.shape != fwd.shape or weights.shape != (10, S):
        raise RuntimeError("tss_reduce: shape mismatch")
    fwd, rc, weights = fwd.contiguous(), rc.contiguous(), weights.contiguous()
    if out is None:
        out = torch.empty((G, 10 * F), dtype=torch.float64, device=fwd.device)
    _lib.call("expecto_tss_reduce", _lib.dptr(fwd), _lib.dptr(rc), _lib.dptr(weights), G, S, F, _lib.dptr(out),
              what="tss_reduce")
    return out


def fwd_rc_average(x: torch.Tensor, out: torch.Tensor | None = None):
    """[2N, F] fp32 -> [N, F]: (x[:N] + x[N:]) / 2 (predict.py:186)."""
    x = x.contiguous()
    n = x.shape[0] // 2
    F = x.shape[1]
    if out is None:
        out = torch.empty((n, F), dtype=x.dtype, device=x.device)
    _lib.call("expecto_fwd_rc_average", _lib.dptr(x), n, F, _lib.dptr(out), what="fwd_rc_average")
    return out


def variant_features(effects: torch.Tensor, dist, strand_plus, shifts, out: torch.Tensor | None = None):
    """effects [S, n, F] fp32 (device, fwd/rc averaged, shift order), dist [n] (pos - TSS),
    strand_plus [n] bool -> [n, 10*F] fp64 (predict.py:87-124 layout: index k*F + f)."""
    return variant_reduce(effects, variant_tables(dist, strand_plus, shifts, effects.device), out)


def variant_tables(dist, strand_plus, shifts, device) -> tuple:
    """The per-batch inputs of ``variant_reduce`` on the device: dist [n] int64, strand [n] u8,
    shifts [S] int32 and the host exp table ``decay_table`` (numpy's exp, as the reference)."""
    d = torch.as_tensor(np.asarray(dist, np.int64), device=device)
    sp = torch.as_tensor(np.asarray(strand_plus, np.uint8), device=device)
    sh = torch.as_tensor(np.asarray(list(shifts), np.int32), device=device)
    lut = torch.from_numpy(decay_table(dist, strand_plus, shifts)).to(device)
    return d, sp, sh, lut


def variant_reduce(effects: torch.Tensor, tables: tuple, out: torch.Tensor | None = None):
    """``variant_features`` on tables already resident (``variant_tables``): one launch per
    65,535 variants (the grid's y limit)."""
    S, n, F = effects.shape
    d, sp, sh, lut = tables
    if d.shape != (n,) or sp.shape != (n,) or sh.shape != (S,):
        raise RuntimeError("variant_reduce: table shapes do not match the effects")
    effects = effects.contiguous()
    if out is None:
        out = torch.empty((n, 10 * F), dtype=torch.float64, device=effects.device)
    for v0 in range(0, n, 65535):
        v1 = min(n, v0 + 65535)
        eff = effects[:, v0:v1].contiguous() if (v0 or v1 != n) else effects
        _lib.call("expecto_variant_reduce_lut", _lib.dptr(eff), _lib.dptr(d[v0:v1]), _lib.dptr(sp[v0:v1]),
                  _lib.dptr(sh), S, v1 - v0, F, _lib.dptr(lut), lut.shape[1], _lib.dptr(out[v0:v1]),
                  what="variant_reduce")
    return out


Contributions = namedtuple("Contributions", "contrib total prop clu clu_prop")


def clusters_csr(clusters, nk: int) -> tuple:
    """Lists of mark indices (0..nk-1), one per cluster -> CSR (ptr int32[n_clu+1], mark int32[...])."""
    ptr = np.zeros(len(clusters) + 1, np.int32)
    ptr[1:] = np.cumsum([len(c) for c in clusters])
    mark = np.asarray([i for c in clusters for i in c], np.int32).reshape(-1)
    if mark.size and (mark.min() < 0 or mark.max() >= nk):
        raise RuntimeError(f"variant_contributions: cluster members must index the {nk} kept marks")
    return ptr, mark


def variant_contributions(eff_ref: torch.Tensor, eff_alt: torch.Tensor, dist, strand_plus, shifts, keep_idx, weights,
                          clusters=None, outputs=None) -> Contributions:
    """Per-mark and per-cluster attribution of the expression effect
    (``predict_by_cluster_rsat.py:105-144``), fused with the spatial reduction
    (``expecto_variant_contrib``; include/expecto_hip.h states the summation order).

    eff_ref, eff_alt ``[S, n, F]`` fp32 (device, fwd/rc averaged, shift order); dist, strand_plus,
    shifts as ``variant_features``; keep_idx: the kept mark columns, ascending; weights
    ``[n_models, 10*nk]`` (or ``[10*nk]``) float64 as ``GBLinear.dump_weights`` gives them;
    clusters: lists of indices into the kept marks, or None.  Returns float64 device tensors
    ``contrib [M, n, nk]``, ``total [M, n]``, ``prop [M, n, nk]``, ``clu`` and ``clu_prop``
    ``[M, n, n_clu]`` (None without clusters); one launch per 65,535 variants.  outputs: the
    names of the tensors wanted (default: all); the others are neither allocated nor written
    and come back as None."""
    S, n, F = eff_ref.shape
    if eff_alt.shape != eff_ref.shape or eff_ref.dtype != torch.float32 or eff_alt.dtype != torch.float32:
        raise RuntimeError("variant_contributions: eff_ref and eff_alt must be fp32 tensors of one shape")
    dev = eff_ref.device
    keep = np.ascontiguousarray(keep_idx, np.int32).reshape(-1)
    nk = keep.size
    if nk == 0 or keep.min() < 0 or keep.max() >= F or np.any(np.diff(keep) <= 0):
        raise RuntimeError("variant_contributions: keep_idx must be ascending mark columns")
    w = torch.as_tensor(weights, dtype=torch.float64).reshape(-1, 10 * nk).contiguous().to(dev)
    M = w.shape[0]
    if M == 0:
        raise RuntimeError("variant_contributions: no model weights")
    d, sp, sh, lut = variant_tables(dist, strand_plus, shifts, dev)
    if d.shape != (n,) or sp.shape != (n,) or sh.shape != (S,):
        raise RuntimeError("variant_contributions: table shapes do not match the effects")
    keep_d = torch.from_numpy(keep).to(dev)
    n_clu, ptr_d, mark_d = 0, None, None
    if clusters is not None:
        ptr, mark = clusters_csr(clusters, nk)
        n_clu = len(ptr) - 1
        ptr_d = torch.from_numpy(ptr).to(dev)
        mark_d = torch.from_numpy(np.concatenate([mark, np.zeros(1, np.int32)])).to(dev)   # never empty
    eff_ref, eff_alt = eff_ref.contiguous(), eff_alt.contiguous()
    wanted = set(Contributions._fields if outputs is None else outputs)
    if not wanted <= set(Contributions._fields):
        raise RuntimeError(f"variant_contributions: outputs are among {Contributions._fields}")
    if not n_clu:
        wanted -= {"clu", "clu_prop"}

    def alloc(rows):
        shapes = {"contrib": (M, rows, nk), "total": (M, rows), "prop": (M, rows, nk), "clu": (M, rows, n_clu),
                  "clu_prop": (M, rows, n_clu)}
        return Contributions(*[torch.empty(shapes[k], dtype=torch.float64, device=dev) if k in wanted else None
                               for k in Contributions._fields])

    def optr(t):
        return None if t is None else _lib.dptr(t)

    out = alloc(n)
    for v0 in range(0, n, 65535):
        v1 = min(n, v0 + 65535)
        whole = v0 == 0 and v1 == n
        er, ea = (eff_ref, eff_alt) if whole else (eff_ref[:, v0:v1].contiguous(), eff_alt[:, v0:v1].contiguous())
        part = out if whole else alloc(v1 - v0)       # the kernel's rows are m * (v1 - v0) + v
        _lib.call(
            "expecto_variant_contrib", _lib.dptr(er), _lib.dptr(ea), _lib.dptr(d[v0:v1]), _lib.dptr(sp[v0:v1]),
            _lib.dptr(sh), S, v1 - v0, F, _lib.dptr(lut), lut.shape[1], _lib.dptr(keep_d), nk, _lib.dptr(w), M,
            _lib.dptr(ptr_d) if n_clu else None, _lib.dptr(mark_d) if n_clu else None, n_clu,
            optr(part.contrib), optr(part.total), optr(part.prop), optr(part.clu), optr(part.clu_prop),
            what="variant_contrib")
        if not whole:
            for dst, src in zip(out, part):
                if dst is not None:
                    dst[:, v0:v1] = src
    return out


def decay_table(dist, strand_plus, shifts) -> np.ndarray:
    """[5, K] float64 exp(-c_k * fl) for fl = 0..K-1, K covering every floor(|d|/200) of the
    batch (d = dist*sgn + shift*sgn): numpy's exp of the arguments predict.py:88-107 passes it,
    so the device reduction reproduces the reference's weights exactly."""
    sgn = np.where(np.asarray(strand_plus, bool), 1, -1).astype(np.int64)
    d = np.asarray(dist, np.int64) * sgn
    sh = np.asarray(list(shifts), np.int64)
    reach = int(np.abs(d).max(initial=0)) + int(np.abs(sh).max(initial=0))
    fl = np.arange(int(np.floor(reach / 200.0)) + 1, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.exp(-c * fl) for c in (0.01, 0.02, 0.05, 0.1, 0.2)]))
