"""Empirical significance of variant effects against a background variant set (e-values).

    python -m expecto_amd.significance build --snpEffectFile bg/snps.shift_0.diff.h5 [more files...] \\
        [--belugaFeatures resources/deepsea_beluga_2002_features.tsv] -o background.h5
    python -m expecto_amd.significance score --background background.h5 \\
        --snpEffectFile out/snps.shift_0.diff.h5 --coorFile_chromatin snps_hg19.vcf \\
        --belugaFeatures resources/deepsea_beluga_2002_features.tsv [--no_tf_features ...] \\
        [--alpha 0.01] [--write-evalues] -o OUT

``expecto_amd.chromatin`` writes raw ``alt - ref`` probability differences, which cannot be compared
across marks: a 0.01 shift of a saturated DNase track is routine, the same shift of a rare TF track
is extreme.  Against a background of B variants (the effects of a large variant set through the same
model), the e-value of an effect on mark c is the add-one fraction of the background whose effect
on c is at least as large:

    ge[v, j] = #{b : |bg[b, cols[j]]| >= |x[v, cols[j]]|}     exact, ties count
    e[v, j]  = (ge + 1) / (B + 1)                              float64

and per variant ``mean_neg_log10_e``, ``max_neg_log10_e``, the mark of the smallest e-value and the
number of marks with ``e <= alpha`` (``ge + 1 <= floor(alpha * (B + 1))``, an integer comparison).
include/expecto_hip.h states the definitions and the summation order.  They are this project's: the
reference has no script for them and no published e-value table is reproduced.

The effect of a variant is the fwd/rc average of the ``diff`` dataset (``features.fwd_rc_average``).
``build`` sorts the magnitudes per mark once (``torch.sort``: plumbing); ``score`` runs
``expecto_ecdf_tail_counts`` and ``expecto_ecdf_summary``.  Nothing here is specific to the 2002
Beluga marks: a ``[n, models]`` SED matrix against a SED background works unchanged.  There is no
CPU path.
"""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib

SORT_BLOCK = 256        # marks sorted per torch.sort call


def neg_log10_table(B: int) -> np.ndarray:
    """float64 [B + 1]: ``-log10((k + 1) / (B + 1))`` by numpy on the host (the device log differs in
    the last ulp)."""
    return -np.log10((np.arange(B + 1, dtype=np.float64) + 1.0) / (B + 1.0))


class Background:
    """The sorted background: ``sorted`` float32 ``[C, B]`` on the device, ascending per mark;
    ``features``: the C mark names (bytes)."""

    def __init__(self, sorted_, features=None):
        if sorted_.dim() != 2 or sorted_.shape[1] < 1 or sorted_.shape[0] < 1:
            raise ValueError("Background: sorted must be [C, B] with B >= 1")
        self.sorted = sorted_.contiguous()
        C = self.sorted.shape[0]
        feats = [f"mark{i}" for i in range(C)] if features is None else list(features)
        if len(feats) != C:
            raise ValueError(f"Background: {len(feats)} feature names for {C} marks")
        self.features = [f if isinstance(f, bytes) else str(f).encode() for f in feats]
        self._lut = None

    @property
    def C(self) -> int:
        return int(self.sorted.shape[0])

    @property
    def n(self) -> int:
        return int(self.sorted.shape[1])

    def lut(self):
        """``neg_log10_table(B)`` on the background's device, uploaded once."""
        if self._lut is None:
            self._lut = _lib.upload(neg_log10_table(self.n), self.sorted.device)
        return self._lut

    def save(self, path: str) -> None:
        from . import h5
        h5.write(path, {"sorted": self.sorted.cpu().numpy(), "features": np.array(self.features),
                        "n": np.float64(self.n)})

    @classmethod
    def load(cls, path: str, device=None) -> "Background":
        from . import h5
        _lib.require_gpu("significance")
        d = h5.read(path)
        s = np.ascontiguousarray(d["sorted"], np.float32)
        if s.ndim != 2 or int(d["n"]) != s.shape[1]:
            raise ValueError(f"{path}: sorted {s.shape} does not match n = {d['n']}")
        return cls(_lib.upload(s, _lib.device_of(device)), [bytes(f) for f in np.asarray(d["features"]).reshape(-1)])


def build_background(effects, features=None) -> Background:
    """``effects``: float32 ``[B, C]`` device tensor, one row per background variant.  Magnitudes,
    sorted ascending per mark, ``SORT_BLOCK`` marks per ``torch.sort``; a NaN is refused."""
    torch = _lib.require_gpu("significance")
    if not effects.is_cuda or effects.dtype != torch.float32 or effects.dim() != 2 or effects.shape[0] < 1:
        raise ValueError("build_background: effects must be a float32 [B >= 1, C] device tensor")
    if bool(torch.isnan(effects).any()):
        raise ValueError("build_background: NaN in the background effects")
    B, C = effects.shape
    out = torch.empty((C, B), dtype=torch.float32, device=effects.device)
    for c0 in range(0, C, SORT_BLOCK):
        block = effects[:, c0:c0 + SORT_BLOCK].abs().T.contiguous()
        out[c0:c0 + SORT_BLOCK] = torch.sort(block, dim=1).values
    return Background(out, features)


@dataclass
class Significance:
    """Device tensors: ``ge`` int32 ``[n, nc]``; ``mean_nlog``, ``max_nlog`` float64 ``[n]``; ``top``
    (an index into ``cols``) and ``n_sig`` int32 ``[n]``.  ``cols``: the host int32 column map;
    ``B``: the background size."""
    ge: object
    mean_nlog: object
    max_nlog: object
    top: object
    n_sig: object
    cols: np.ndarray
    B: int

    def evalues(self):
        """float64 ``[n, nc]`` device tensor ``(ge + 1) / (B + 1)``; NaN for a NaN query."""
        # gathered from the B + 2 values numpy divides on the host (slot 0: NaN), as nlog is from its
        # table: torch divides a tensor by a scalar through the reciprocal, which is an ulp off
        table = np.concatenate([[np.nan], (np.arange(self.B + 1, dtype=np.float64) + 1.0) / (self.B + 1.0)])
        return _lib.upload(table, self.ge.device)[(self.ge + 1).long()]


def _columns(bg: Background, x, cols):
    torch = _lib.require_gpu("significance")
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("significance: x must be a float32 [n, marks] device tensor")
    if x.device != bg.sorted.device:
        raise ValueError("significance: x and the background live on different devices")
    cols = np.arange(bg.C, dtype=np.int32) if cols is None else np.ascontiguousarray(cols, np.int32).reshape(-1)
    if cols.size < 1 or cols.min() < 0 or cols.max() >= bg.C or np.any(np.diff(cols) <= 0):
        raise ValueError(f"significance: cols must be ascending mark indices in 0..{bg.C - 1}")
    if x.shape[1] <= int(cols.max()):
        raise ValueError(f"significance: x has {x.shape[1]} columns, cols reaches {int(cols.max())}")
    if x.shape[0] and x.stride(1) != 1:
        x = x.contiguous()
    return x, cols


def tail_counts(bg: Background, x, cols=None):
    """int32 ``[n, nc]`` device tensor of ``ge`` (module docstring); ``x`` float32 ``[n, >= max(cols) + 1]``
    on the background's device, rows of any stride; ``cols``: ascending mark indices (default: all)."""
    import torch
    x, cols = _columns(bg, x, cols)
    n = int(x.shape[0])
    ge = torch.empty((n, cols.size), dtype=torch.int32, device=x.device)
    cols_d = _lib.upload(cols, x.device)
    _lib.call("expecto_ecdf_tail_counts", _lib.dptr(bg.sorted), bg.n, bg.C, cols.ctypes.data, _lib.dptr(cols_d),
              int(cols.size), _lib.dptr(x), int(x.stride(0)) if n else int(cols.max()) + 1, n, _lib.dptr(ge),
              what="ecdf_tail_counts")
    return ge


def score(bg: Background, x, cols=None, alpha: float = 0.01) -> Significance:
    """Tail counts and per-variant summaries of ``x`` against ``bg`` at level ``alpha``."""
    import torch
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("significance: alpha must lie in [0, 1]")
    x, cols = _columns(bg, x, cols)
    ge = tail_counts(bg, x, cols)
    n, dev = int(ge.shape[0]), ge.device
    mean, mx = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    top, n_sig = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    k_alpha = int(np.floor(alpha * (bg.n + 1)))
    _lib.call("expecto_ecdf_summary", _lib.dptr(ge), n, int(cols.size), _lib.dptr(bg.lut()), bg.n, k_alpha,
              _lib.dptr(mean), _lib.dptr(mx), _lib.dptr(top), _lib.dptr(n_sig), what="ecdf_summary")
    return Significance(ge, mean, mx, top, n_sig, cols, bg.n)


# ---------------------------------------------------------------------------- files
def read_effects(paths, device=None):
    """The fwd/rc-averaged ``diff`` rows of one or more ``.diff.h5`` files, concatenated: float32
    ``[N, F]`` on the device."""
    import torch

    from . import h5
    from .features import fwd_rc_average
    dev = _lib.device_of(device)
    parts = []
    for p in paths:
        d = np.ascontiguousarray(h5.read(p)["diff"], np.float32)
        if d.ndim != 2 or d.shape[0] % 2:
            raise ValueError(f"{p}: diff must hold the forward rows then the reverse-complement rows")
        parts.append(fwd_rc_average(_lib.upload(d, dev)))
    return torch.cat(parts, 0) if len(parts) > 1 else parts[0]


def _coor_header(k: int) -> list:
    return (["chrom", "pos", "id", "ref", "alt"] + [f"col{i}" for i in range(5, k)])[:k]


def write_table(path: str, coor, sig: Significance, names) -> None:
    """``significance.tsv``: the coordinate columns, then mean_neg_log10_e, max_neg_log10_e (``repr``
    of the float64), top_feature (a name of ``names``, one per scored column) and n_significant."""
    mean, mx = sig.mean_nlog.cpu().numpy(), sig.max_nlog.cpu().numpy()
    top, n_sig = sig.top.cpu().numpy(), sig.n_sig.cpu().numpy()
    rows = coor.astype(str).values.tolist()
    with open(path, "w") as f:
        f.write("\t".join(_coor_header(coor.shape[1]) + ["mean_neg_log10_e", "max_neg_log10_e", "top_feature",
                                                         "n_significant"]) + "\n")
        for i, r in enumerate(rows):
            name = names[top[i]] if top[i] >= 0 else "NA"
            f.write("\t".join(r + [repr(float(mean[i])), repr(float(mx[i])), name, str(int(n_sig[i]))]) + "\n")


# ---------------------------------------------------------------------------- CLI
def build_parser():
    p = argparse.ArgumentParser(description="Empirical significance of variant effects against a background")
    sub = p.add_subparsers(dest="command", required=True)
    b = sub.add_parser("build", help="sort the effects of a background variant set per mark")
    b.add_argument("--snpEffectFile", nargs="+", required=True, dest="snpEffectFile",
                   help=".diff.h5 files of the background (the --chunk_i outputs of chromatin are concatenated)")
    b.add_argument("--belugaFeatures", dest="belugaFeatures", default=None,
                   help="tsv file denoting the features: their names are stored with the background")
    b.add_argument("-o", dest="out", required=True, help="background.h5")
    s = sub.add_parser("score", help="e-values and per-variant summaries of a .diff.h5 against a background")
    s.add_argument("--background", required=True)
    s.add_argument("--snpEffectFile", required=True, dest="snpEffectFile")
    s.add_argument("--coorFile_chromatin", required=True, dest="coorFile_chromatin")
    s.add_argument("--belugaFeatures", required=True, dest="belugaFeatures")
    for flag in ("no_tf_features", "no_dnase_features", "no_histone_features", "intersect_with_lambert", "no_pol2"):
        s.add_argument("--" + flag, action="store_true", dest=flag, default=False)
    s.add_argument("--alpha", type=float, default=0.01)
    s.add_argument("--write-evalues", action="store_true", dest="write_evalues")
    s.add_argument("-o", dest="out_dir", required=True)
    return p


def feature_names(path: str) -> list:
    from . import predict
    return list(predict.read_features_table(path)["Assay type + assay + cell type"].astype(str))


def run_build(args) -> Background:
    eff = read_effects(args.snpEffectFile)
    names = feature_names(args.belugaFeatures) if args.belugaFeatures else None
    bg = build_background(eff, names)
    bg.save(args.out)
    print(f"background of {bg.n} variants x {bg.C} marks -> {args.out}")
    return bg


def run_score(args) -> Significance:
    import pandas as pd

    from . import h5, predict
    bg = Background.load(args.background)
    feats = predict.read_features_table(args.belugaFeatures)
    if feats.shape[0] != bg.C:
        raise ValueError(f"{args.belugaFeatures}: {feats.shape[0]} features, the background has {bg.C} marks")
    cols = np.nonzero(predict.get_keep_mask(feats, *predict.mask_arguments(args)))[0].astype(np.int32)
    names = list(feats["Assay type + assay + cell type"].astype(str).values[cols])
    x = read_effects([args.snpEffectFile], bg.sorted.device)
    coor = pd.read_csv(args.coorFile_chromatin, sep="\t", header=None, comment="#", dtype=str, keep_default_na=False)
    if coor.shape[0] != x.shape[0]:
        raise ValueError(f"{args.coorFile_chromatin}: {coor.shape[0]} variants, {args.snpEffectFile} holds {x.shape[0]}")
    sig = score(bg, x, cols, args.alpha)
    os.makedirs(args.out_dir, exist_ok=True)
    write_table(os.path.join(args.out_dir, "significance.tsv"), coor, sig, names)
    if args.write_evalues:
        h5.write(os.path.join(args.out_dir, "evalues.h5"), {"evalue": sig.evalues().cpu().numpy()})
    return sig


def main(argv=None):
    args = build_parser().parse_args(argv)
    _lib.require_gpu("significance")
    return run_build(args) if args.command == "build" else run_score(args)


if __name__ == "__main__":
    main(sys.argv[1:])
