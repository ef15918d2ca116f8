"""CPU restatement of the code-producing kernels of reduce.hip -- TEST INFRASTRUCTURE (oracle) ONLY.

Written from the contracts in ``include/expecto_hip.h``, one position at a time, with none of
the kernels' packing or index arithmetic.  ``genome`` is a 1-D uint8 array of base codes
(0=A 1=G 2=C 3=T 4=zero column); a position outside ``[0, len(genome))`` reads as code 4.

* ``variant_windows`` -- ``expecto_variant_windows`` (chromatin.py:202-209 + the crop of :164).
* ``tss_windows``     -- ``expecto_tss_windows`` (compute_expecto_features.py:107-111).
* ``gather_segments`` -- ``expecto_gather_segments``.
* ``indel_windows``   -- ``expecto_indel_windows``: the spliced sequence as a concatenation,
                         then the centre crop.
"""
from __future__ import annotations

import numpy as np

LEN = 2000
OUTSIDE = 4


def read(genome: np.ndarray, start: int, length: int) -> np.ndarray:
    """``length`` codes from position ``start``; positions outside the genome read as 4."""
    start, length = int(start), int(length)
    out = np.full(length, OUTSIDE, np.uint8)
    lo, hi = max(start, 0), min(start + length, int(genome.shape[0]))
    if lo < hi:
        out[lo - start:hi - start] = genome[lo:hi]
    return out


def variant_windows(genome, var_off, ref_code, alt_code, shifts) -> np.ndarray:
    """uint8 [2, S, n, 2000]: allele a, shift j, variant v holds genome[off_v + shift - 999 + i]
    with the code at i = 999 - shift (where it lies inside the window) replaced by the allele's."""
    n, S = len(var_off), len(shifts)
    out = np.empty((2, S, n, LEN), np.uint8)
    for a, allele in enumerate((ref_code, alt_code)):
        for j, sh in enumerate(shifts):
            for v in range(n):
                w = read(genome, int(var_off[v]) + int(sh) - 999, LEN)
                m = 999 - int(sh)
                if 0 <= m < LEN:
                    w[m] = allele[v]
                out[a, j, v] = w
    return out


def tss_windows(genome, tss_off, strand, shifts) -> np.ndarray:
    """uint8 [G, S, 2000]: gene g, shift j covers tss_off[g] + shifts[j]*strand[g] - 999 + i."""
    G, S = len(tss_off), len(shifts)
    out = np.empty((G, S, LEN), np.uint8)
    for g in range(G):
        for j, sh in enumerate(shifts):
            out[g, j] = read(genome, int(tss_off[g]) + int(sh) * int(strand[g]) - 999, LEN)
    return out


def gather_segments(genome, start, seg_len, splice_pos=None, splice_code=None) -> np.ndarray:
    """uint8 [n, seg_len]: genome[start[i] + j], with index splice_pos[i] (where it lies inside
    the segment) set to splice_code[i] when splice_code is given."""
    n = len(start)
    out = np.empty((n, seg_len), np.uint8)
    for i in range(n):
        s = read(genome, int(start[i]), seg_len)
        if splice_code is not None and 0 <= int(splice_pos[i]) < seg_len:
            s[int(splice_pos[i])] = splice_code[i]
        out[i] = s
    return out


def indel_windows(genome, start0, mutpos, lref, lalt, crop, alleles) -> np.ndarray:
    """uint8 [n, 2000]: item t's 2100-base fetch window starts at start0[t]; alleles[t] (lalt[t]
    codes) replaces lref[t] bases at mutpos[t]; the output is 2000 codes of the spliced sequence
    from crop[t] on.  For 0 <= mutpos, mutpos + lref <= 2100 and a spliced length >= 2000 (the
    items the device takes)."""
    n = len(start0)
    out = np.empty((n, LEN), np.uint8)
    for t in range(n):
        win = [int(c) for c in read(genome, int(start0[t]), LEN + 100)]
        mp, lr = int(mutpos[t]), int(lref[t])
        allele = [int(c) for c in alleles[t]]
        assert len(allele) == int(lalt[t]) and 0 <= mp and mp + lr <= LEN + 100
        spliced = win[:mp] + allele + win[mp + lr:]
        assert len(spliced) >= LEN + int(crop[t])
        out[t] = spliced[int(crop[t]):int(crop[t]) + LEN]
    return out
