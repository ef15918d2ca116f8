"""Drop-in for the reference ``query_fimo_for_predictions.py``: which motifs match the reference genome at
each variant?  The reference writes the +-30 bp flanks to a FASTA file, runs the MEME suite's
``fimo --thresh 1 --text`` on it, and keeps, of that table, the rows that overlap the variant and of those
the best per (motif, variant).  Here FIMO's scoring model runs on the device and only the windows that
cover the variant are ever scored (``expecto_pwm_pvalues``, ``expecto_pwm_scan``: include/expecto_hip.h).

    python -m expecto_amd.query_fimo_for_predictions --vcf_file V --motif_file M.meme [--chunk_size N --chunk_i I] \\
        [--bp_pad 30] [--hg19_fasta resources/hg19.fa] [--bgfile nrdb] [--motif-pseudo 0.1] [--thresh 1.0] \\
        [--seq-batch 8192] [-o temp_query_fimo_for_predictions]

Writes ``fimo_filtered.tsv`` (the reference's layout) and ``fimo_out.txt`` (the same rows under a ``#``
header, plus the best row of every motif that has none, so that every motif is named: what
``cluster_analysis_with_fimo --fimo_out_file`` needs).  ``--thresh 1`` keeps a row for every (motif, variant)
pair, as the reference does; a threshold near the later ``--pval_match_threshold`` keeps the files small.

The model (INTEGRATION.md lists the differences from the ``fimo`` binary, against which nothing here has
been measured: it is not part of this project).  Letters are in alphabet order A C G T in this module's
arguments; the packed matrix of :class:`Motifs` is in base-code order (0=A 1=G 2=C 3=T).

* background: made strand-symmetric, ``A = T = (A + T) / 2``, ``C = G = (C + G) / 2``;
* ``f = (freq * nsites + pseudo * bg) / (nsites + pseudo)``, ``lo = log2(f / bg)``; ``mn``, ``mx`` over the
  matrix (``mn = mx - 1`` when equal), ``scale = 100 / (mx - mn)``, ``offset = mn``, scaled entry
  ``rint((lo - offset) * scale)`` in 0..100; a match's raw score is ``scaled_sum / scale + w * offset``;
* p-value of a scaled sum: the tail of the exact distribution of the sum under the background;
* per (sequence, motif) the window of maximal scaled sum among those that cover the variant and hold
  no non-ACGT base, both strands; equal sums to the smaller start, then to ``+``.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
from typing import NamedTuple

import numpy as np

from .cluster_analysis_with_fimo import FIMO_COLUMNS

MAX_W, MAX_L, RANGE = 64, 256, 100           # include/expecto_hip.h
ALPHABET = "ACGT"
TO_CODE_ORDER = [0, 2, 1, 3]                 # alphabet column of code 0..3 (A G C T)
NRDB = (0.281774, 0.222020, 0.228876, 0.267330)     # FIMO's built-in default: from memory, unverified
_COMPLEMENT = str.maketrans("ACGT", "TGCA")


class Meme(NamedTuple):
    background: object         # float64 [4] in alphabet order as the file gives it, or None
    ids: list
    alt_ids: list              # "" where the MOTIF line has none
    freqs: list                # float64 [w, 4] per motif, alphabet order
    nsites: list               # float; 20 where missing or <= 0


class Motifs(NamedTuple):
    """The motifs of a scan, packed for the device."""
    ids: list
    alt_ids: list
    pssm: np.ndarray           # int16 [col_ptr[M], 4]: scaled entries, base-code order
    col_ptr: np.ndarray        # int32 [M + 1]
    scales: np.ndarray         # float64 [M]
    offsets: np.ndarray        # float64 [M]

    @property
    def widths(self):
        return np.diff(self.col_ptr)

    def __len__(self):
        return len(self.ids)

    @classmethod
    def from_meme(cls, meme: Meme, bg, pseudo: float = 0.1) -> "Motifs":
        mats, scales, offsets = [], [], []
        for name, f, n in zip(meme.ids, meme.freqs, meme.nsites):
            if not 1 <= f.shape[0] <= MAX_W:
                raise ValueError(f"motif {name}: width {f.shape[0]}; supported are 1..{MAX_W}")
            m, sc, off = build_pssm(f, n, bg, pseudo)
            mats.append(m[:, TO_CODE_ORDER])
            scales.append(sc)
            offsets.append(off)
        col_ptr = np.zeros(len(mats) + 1, np.int32)
        col_ptr[1:] = np.cumsum([m.shape[0] for m in mats])
        pssm = np.concatenate(mats).astype(np.int16) if mats else np.zeros((0, 4), np.int16)
        return cls(list(meme.ids), list(meme.alt_ids), np.ascontiguousarray(pssm), col_ptr,
                   np.array(scales, np.float64), np.array(offsets, np.float64))


class Tables(NamedTuple):
    """Device side of :class:`Motifs`: the matrix, its column offsets and the p-value tables."""
    pssm: object               # int16 [total, 4]
    col_ptr: object            # int32 [M + 1]
    tables: object             # float64 [100 total + M]
    pv_ptr: object             # int64 [M + 1]


# ---- motifs -----------------------------------------------------------------------------------

def _letter_freqs(tokens, what):
    """``A 0.25 C 0.25 ...`` -> float64 [4] in alphabet order."""
    got = {}
    for k, v in zip(tokens[0::2], tokens[1::2]):
        got[k.upper()] = float(v)
    if sorted(got) != sorted(ALPHABET) or len(tokens) != 8:
        raise ValueError(f"{what}: expected a frequency for each of A C G T, got {' '.join(tokens)!r}")
    return np.array([got[a] for a in ALPHABET], np.float64)


def read_meme(path: str) -> Meme:
    """The minimal MEME text format: the ``Background letter frequencies`` line and the one after it,
    ``MOTIF <id> [<alt>]``, and ``letter-probability matrix: alength= 4 w= W nsites= N ...`` with its W rows.
    Everything else is passed over."""
    with open(path) as f:
        lines = [ln.strip() for ln in f]
    background, ids, alts, freqs, nsites = None, [], [], [], []
    name, i = None, 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        if ln.startswith("Background letter frequencies"):
            if i >= len(lines):
                raise ValueError(f"{path}: no line after 'Background letter frequencies'")
            background = _letter_freqs(lines[i].split(), f"{path}: background")
            i += 1
        elif ln.startswith("MOTIF"):
            tok = ln.split()
            if len(tok) < 2:
                raise ValueError(f"{path}: MOTIF line without an id")
            if name is not None:
                raise ValueError(f"motif {name[0]}: no letter-probability matrix")
            name = (tok[1], tok[2] if len(tok) > 2 else "")
        elif ln.startswith("letter-probability matrix"):
            if name is None:
                raise ValueError(f"{path}: letter-probability matrix before any MOTIF line")
            keys = dict(re.findall(r"(\w+)=\s*(\S+)", ln))
            if int(keys.get("alength", 4)) != 4:
                raise ValueError(f"motif {name[0]}: alength= {keys['alength']}; only 4 letters (DNA) are supported")
            rows = []
            want = int(keys["w"]) if "w" in keys else None
            while i < len(lines) and (want is None or len(rows) < want):
                tok = lines[i].split()
                try:
                    row = [float(t) for t in tok]
                except ValueError:
                    break
                if len(row) != 4:
                    break
                rows.append(row)
                i += 1
            if not rows or (want is not None and len(rows) < want):
                raise ValueError(f"motif {name[0]}: {len(rows)} matrix rows of 4 numbers, w= {want}")
            m = np.array(rows, np.float64)
            bad = np.nonzero(np.abs(m.sum(axis=1) - 1.0) > 1e-2)[0]
            if bad.size:
                raise ValueError(f"motif {name[0]}: row {int(bad[0]) + 1} sums to {m[bad[0]].sum():g}, not 1")
            n = float(keys.get("nsites", 0))
            ids.append(name[0])
            alts.append(name[1])
            freqs.append(m)
            nsites.append(n if n > 0 else 20.0)
            name = None
    if name is not None:
        raise ValueError(f"motif {name[0]}: no letter-probability matrix")
    return Meme(background, ids, alts, freqs, nsites)


def symmetric(bg) -> np.ndarray:
    """``A = T = (A + T) / 2``, ``C = G = (C + G) / 2`` of a float64 [4] in alphabet order."""
    bg = np.asarray(bg, np.float64)
    at, cg = (bg[0] + bg[3]) / 2, (bg[1] + bg[2]) / 2
    return np.array([at, cg, cg, at], np.float64)


def background(spec: str, meme: Meme | None = None) -> np.ndarray:
    """``--bgfile``: ``nrdb``, ``motif-file``, ``uniform`` or the path of a file of ``A 0.29`` lines.  The
    result is strand-symmetric, float64 [4] in alphabet order."""
    if spec == "nrdb":
        bg = np.array(NRDB, np.float64)
    elif spec == "uniform":
        bg = np.full(4, 0.25)
    elif spec == "motif-file":
        if meme is None or meme.background is None:
            raise ValueError("--bgfile motif-file: the motif file has no 'Background letter frequencies'")
        bg = meme.background
    else:
        tokens = []
        with open(spec) as f:
            for ln in f:
                ln = ln.split("#")[0].split()
                if len(ln) == 2 and len(ln[0]) == 1:       # longer words are higher-order entries
                    tokens += ln
        bg = _letter_freqs(tokens, spec)
    if not (np.isfinite(bg).all() and (bg > 0).all()):
        raise ValueError(f"background {bg.tolist()}: every frequency must be positive")
    return symmetric(bg)


def _checked_bg(bg) -> np.ndarray:
    bg = np.asarray(bg, np.float64)
    if bg.shape != (4,) or not (bg > 0).all() or not (bg < 1).all():
        raise ValueError(f"bg must be four frequencies in (0, 1), got {bg!r}")
    if bg[0] != bg[3] or bg[1] != bg[2]:
        raise ValueError(f"bg {bg.tolist()} is not strand-symmetric (A = T and C = G): see symmetric()")
    return bg


def build_pssm(freqs, nsites, bg, pseudo: float = 0.1):
    """``(int64 [w, 4] in 0..100, scale, offset)`` of a frequency matrix [w, 4]; alphabet order throughout."""
    bg = _checked_bg(bg)
    freqs = np.asarray(freqs, np.float64)
    if freqs.ndim != 2 or freqs.shape[1] != 4 or freqs.shape[0] < 1:
        raise ValueError(f"freqs has shape {freqs.shape}; expected [w >= 1, 4]")
    nsites, pseudo = float(nsites), float(pseudo)
    f = (freqs * nsites + pseudo * bg) / (nsites + pseudo)
    if not (f > 0).all():
        raise ValueError("a zero frequency with a zero pseudocount has no log-odds score")
    lo = np.log2(f / bg)
    mn, mx = float(lo.min()), float(lo.max())
    if mn == mx:
        mn = mx - 1
    scale, offset = 100 / (mx - mn), mn
    return np.rint((lo - offset) * scale).astype(np.int64), scale, offset


# ---- device -----------------------------------------------------------------------------------

def pvalue_tables(motifs: Motifs, bg, device=None) -> Tables:
    """The motifs on the device with their score-to-p-value tables (one ``expecto_pwm_pvalues`` call)."""
    from . import _lib
    torch = _lib.require_gpu("query_fimo_for_predictions")
    bg = np.ascontiguousarray(_checked_bg(bg)[TO_CODE_ORDER])
    dev = _lib.device_of(device)
    M, total = len(motifs), int(motifs.col_ptr[-1])
    with torch.cuda.device(dev):
        pssm = torch.from_numpy(motifs.pssm).to(dev)
        col_ptr = torch.from_numpy(motifs.col_ptr).to(dev)
        tables = torch.empty(RANGE * total + M, dtype=torch.float64, device=dev)
        pv_ptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        _lib.call("expecto_pwm_pvalues", pssm.data_ptr() if total else None, motifs.col_ptr.ctypes.data,
                  col_ptr.data_ptr(), M, bg.ctypes.data, tables.data_ptr() if M else None, pv_ptr.data_ptr(),
                  int(tables.numel()))
    return Tables(pssm, col_ptr, tables, pv_ptr)


def scan(codes, overlap, motifs: Motifs, tables: Tables):
    """Best match per (sequence, motif): ``(score int32, start int32, strand uint8, pvalue float64)``, device
    tensors [S, M] (one ``expecto_pwm_scan`` call).  codes: uint8 [S, L] base codes (a device tensor with
    contiguous rows is used in place; a host array is uploaded); overlap: one position for all sequences or
    int32 [S], -1 for "any window"."""
    from . import _lib
    torch = _lib.require_gpu("query_fimo_for_predictions")
    dev = tables.tables.device
    if not torch.is_tensor(codes):
        codes = _lib.upload(np.asarray(codes, np.uint8), dev)
    if codes.dtype != torch.uint8 or codes.dim() != 2 or not codes.is_cuda or (codes.shape[1] > 1 and codes.stride(1) != 1):
        raise ValueError("codes must be uint8 [S, L] on the device with contiguous rows")
    S, L = int(codes.shape[0]), int(codes.shape[1])
    if not 1 <= L <= MAX_L:
        raise ValueError(f"scan: sequences of {L} bases; supported are 1..{MAX_L}")
    ld = int(codes.stride(0)) if S > 1 else L
    if np.ndim(overlap) == 0 and not torch.is_tensor(overlap):
        overlap = torch.full((S,), int(overlap), dtype=torch.int32, device=dev)
    elif not torch.is_tensor(overlap):
        overlap = _lib.upload(np.asarray(overlap, np.int32), dev)
    if overlap.dtype != torch.int32 or overlap.shape != (S,) or not overlap.is_contiguous():
        raise ValueError("overlap must be one position or int32 [S]")
    M = len(motifs)
    with torch.cuda.device(dev):
        score = torch.empty((S, M), dtype=torch.int32, device=dev)
        start = torch.empty((S, M), dtype=torch.int32, device=dev)
        strand = torch.empty((S, M), dtype=torch.uint8, device=dev)
        pvalue = torch.empty((S, M), dtype=torch.float64, device=dev)
        if S and M:
            _lib.call("expecto_pwm_scan", codes.data_ptr(), S, L, ld, overlap.data_ptr(), tables.pssm.data_ptr(),
                      motifs.col_ptr.ctypes.data, tables.col_ptr.data_ptr(), M, tables.tables.data_ptr(),
                      tables.pv_ptr.data_ptr(), int(tables.tables.numel()), score.data_ptr(), start.data_ptr(),
                      strand.data_ptr(), pvalue.data_ptr())
    return score, start, strand, pvalue


def matches_csr(pvalue, threshold: float, motif_map=None):
    """``(seq_ptr int64 [S + 1], motif_idx int32)`` of the pairs with ``pvalue < threshold`` (a pair without a
    window, NaN, is none), compacted on the device: what ``cluster_analysis_with_fimo.enrichment`` takes
    as ``matches``.  ``motif_map`` (int [M]) renumbers the motifs; those mapped below 0 are dropped."""
    import torch
    keep = pvalue < float(threshold)
    if motif_map is not None:
        mm = torch.as_tensor(np.asarray(motif_map, np.int64), device=pvalue.device)
        keep &= (mm >= 0)[None, :]
    seq_ptr = torch.zeros(pvalue.shape[0] + 1, dtype=torch.int64, device=pvalue.device)
    seq_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    idx = keep.nonzero()[:, 1]                    # row-major: by sequence, then by motif
    if motif_map is not None:
        idx = mm[idx]
    return seq_ptr.cpu().numpy(), idx.to(torch.int32).cpu().numpy()


# ---- tables -----------------------------------------------------------------------------------

def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def matched_sequence(seq: str, start: int, w: int, strand: int) -> str:
    """The window's bases; on ``-`` their reverse complement, as FIMO prints a match."""
    s = seq[start:start + w]
    return s.translate(_COMPLEMENT)[::-1] if strand else s


def best_matches(names, seqs, motifs: Motifs, score, start, strand, pvalue, thresh: float = 1.0, pairs=None):
    """A DataFrame with FIMO's ten columns, one row per (sequence, motif) that has a window and
    ``p <= thresh``: ``start`` / ``stop`` 1-based inclusive, ``strand`` ``+`` / ``-``, ``score`` the raw score,
    ``p-value`` the exact double, ``q-value`` empty.  Sorted by p-value, then sequence, then motif.
    names, seqs: the sequences' names and (upper-case) bases; the four results [S, M] of :func:`scan`, on the
    device or the host.  ``pairs``: (sequence indices, motif indices) to look at instead of all."""
    import pandas as pd
    score, start, strand, pvalue = (_host(a) for a in (score, start, strand, pvalue))
    if pairs is None:
        si, mi = np.nonzero((score >= 0) & (pvalue <= thresh))
    else:
        si, mi = (np.asarray(p, np.int64) for p in pairs)
        ok = (score[si, mi] >= 0) & (pvalue[si, mi] <= thresh)
        si, mi = si[ok], mi[ok]
    p = pvalue[si, mi]
    order = np.lexsort((mi, si, p))
    si, mi, p = si[order], mi[order], p[order]
    st, sd, sc = start[si, mi].astype(np.int64), strand[si, mi], score[si, mi].astype(np.float64)
    w = motifs.widths[mi].astype(np.int64)
    raw = sc / motifs.scales[mi] + w * motifs.offsets[mi]
    return pd.DataFrame({
        "motif_id": [motifs.ids[m] for m in mi], "motif_alt_id": [motifs.alt_ids[m] for m in mi],
        "sequence_name": [names[s] for s in si], "start": st + 1, "stop": st + w,
        "strand": np.where(sd == 0, "+", "-").astype(object), "score": raw, "p-value": p, "q-value": [""] * len(p),
        "matched_sequence": [matched_sequence(seqs[s], int(a), int(b), int(c)) for s, a, b, c in zip(si, st, w, sd)],
    }, columns=FIMO_COLUMNS)


def _text_rows(df):
    for row in df.itertuples(index=False):
        r = list(row)
        r[6], r[7] = "%g" % r[6], "%.3g" % r[7]
        yield "\t".join(str(x) for x in r)


def write_filtered(df, path: str) -> None:
    """``fimo_filtered.tsv``: the reference's ``to_csv(sep="\\t", header=True)`` layout, the index first; score
    ``%g`` and p-value ``%.3g`` as FIMO's text has them."""
    with open(path, "w") as f:
        f.write("\t" + "\t".join(FIMO_COLUMNS) + "\n")
        f.writelines(f"{i}\t{r}\n" for i, r in enumerate(_text_rows(df)))


def write_fimo_text(df, path: str) -> None:
    """``fimo_out.txt``: FIMO's ``--text`` layout, a ``#`` header and no index."""
    with open(path, "w") as f:
        f.write("# " + "\t".join(FIMO_COLUMNS) + "\n")
        f.writelines(r + "\n" for r in _text_rows(df))


# ---- variants ---------------------------------------------------------------------------------

def read_vcf(path: str, chunk_size=None, chunk_i=None):
    """query_fimo_for_predictions.py:27-31."""
    import pandas as pd
    vcf_df = pd.read_csv(path, sep="\t", comment="#", names=["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"],
                         dtype={"CHROM": str, "ID": str, "REF": str, "ALT": str})
    if chunk_i is not None:
        if not chunk_size or chunk_size < 1:
            raise ValueError("--chunk_i needs a positive --chunk_size")
        vcf_df = vcf_df.iloc[chunk_i * chunk_size:(chunk_i + 1) * chunk_size]
    return vcf_df


def flanks(vcf_df, fasta, pad: int, pad_right=None):
    """``read_seq`` (query_fimo_for_predictions.py:62-70) of every row: ``(names, upper-case sequences, uint8
    codes [S, pad + 1 + pad_right])``, the codes gathered from the genome's code cache.  ``ValueError`` for a
    flank that leaves its contig and for a variant of which neither REF nor ALT is what the genome holds."""
    from .genome import CodeGenome
    pad_right = pad if pad_right is None else pad_right
    L = pad + 1 + pad_right
    if not 1 <= L <= MAX_L:
        raise ValueError(f"flanks of {L} bases; supported are 1..{MAX_L}")
    host = CodeGenome(fasta)
    names, seqs, offs = [], [], np.zeros(len(vcf_df), np.int64)
    for i, (chrom, pos, rsid, ref, alt) in enumerate(zip(vcf_df["CHROM"], vcf_df["POS"], vcf_df["ID"], vcf_df["REF"],
                                                         vcf_df["ALT"])):
        pos = int(pos)
        if chrom not in fasta:
            raise ValueError(f"variant {rsid} ({chrom}:{pos}): no contig {chrom} in the genome")
        if pos - pad < 1 or pos + pad_right > host.lengths[chrom]:
            raise ValueError(f"variant {rsid} ({chrom}:{pos}): the flank {pos - pad}..{pos + pad_right} leaves the "
                             f"contig (1..{host.lengths[chrom]})")
        seq = fasta.sequence({"chr": chrom, "start": pos - pad, "stop": pos + pad_right}).upper()
        ref, alt = str(ref).upper(), str(alt).upper()
        if seq[pad:pad + len(ref)] != ref and seq[pad:pad + len(alt)] != alt:
            raise ValueError(f"variant {rsid} ({chrom}:{pos}): fasta does not match VCF (the genome has "
                             f"{seq[pad:pad + max(len(ref), len(alt))]!r}, REF {ref!r}, ALT {alt!r})")
        names.append(str(rsid))
        seqs.append(seq)
        offs[i] = host.offset(chrom, pos - pad)
    codes = np.asarray(host.codes)[offs[:, None] + np.arange(L)[None, :]] if len(offs) else np.zeros((0, L), np.uint8)
    return names, seqs, np.ascontiguousarray(codes, np.uint8)


# ---- CLI --------------------------------------------------------------------------------------

def build_parser():
    """The arguments of query_fimo_for_predictions.py:11-20, and those the ``fimo`` command line had."""
    parser = argparse.ArgumentParser(prog="python -m expecto_amd.query_fimo_for_predictions",
                                     description='Query FIMO for each SNP in SED df')
    parser.add_argument("--vcf_file", required=True)
    parser.add_argument("--motif_file", required=True)
    parser.add_argument("--chunk_size", action="store", dest="chunk_size", type=int, default=None,
                        help="Size of chunks for batching predictions")
    parser.add_argument("--chunk_i", action="store", dest="chunk_i", type=int, default=None,
                        help="Chunk index for current run, starting from 0")
    parser.add_argument("--bp_pad", type=int, default=30)
    parser.add_argument("--hg19_fasta", default="resources/hg19.fa")
    parser.add_argument("--bgfile", default="nrdb", help="nrdb, motif-file, uniform, or a file of 'A 0.29' lines")
    parser.add_argument("--motif-pseudo", dest="motif_pseudo", type=float, default=0.1)
    parser.add_argument("--thresh", type=float, default=1.0, help="keep the matches with p-value <= this")
    parser.add_argument("--seq-batch", dest="seq_batch", type=int, default=8192, help="sequences per device call")
    parser.add_argument('-o', dest="out_dir", type=str, default='temp_query_fimo_for_predictions', help='Output directory')
    return parser


def run(args):
    """One CLI run; returns the DataFrame of ``fimo_filtered.tsv`` (exact p-values and scores)."""
    import pandas as pd

    from . import _lib
    from .genome import open_genome
    torch = _lib.require_gpu("query_fimo_for_predictions")
    if args.seq_batch < 1:
        raise ValueError("--seq-batch must be at least 1")
    os.makedirs(args.out_dir, exist_ok=True)
    meme = read_meme(args.motif_file)
    bg = background(args.bgfile, meme)
    motifs = Motifs.from_meme(meme, bg, args.motif_pseudo)
    names, seqs, codes = flanks(read_vcf(args.vcf_file, args.chunk_size, args.chunk_i), open_genome(args.hg19_fasta),
                                args.bp_pad)
    tables = pvalue_tables(motifs, bg)
    M = len(motifs)
    parts = []
    best_p = torch.full((M,), float("inf"), dtype=torch.float64, device=tables.tables.device)
    best_s = torch.full((M,), -1, dtype=torch.int64, device=tables.tables.device)
    for s0 in range(0, len(names), args.seq_batch):
        s1 = min(len(names), s0 + args.seq_batch)
        res = scan(codes[s0:s1], args.bp_pad, motifs, tables)
        pv = res[3]
        if M:
            # the motif's best pair of the batch; NaN (no window) never wins, an equal p keeps the earlier variant
            col = torch.where(torch.isnan(pv), torch.full_like(pv, float("inf")), pv)
            lo, at = col.min(dim=0)
            at = (col == lo[None, :]).to(torch.uint8).argmax(dim=0)          # the first of the minimum
            better = lo < best_p
            best_p = torch.where(better, lo, best_p)
            best_s = torch.where(better, at + s0, best_s)
        si, mi = (pv <= args.thresh).nonzero(as_tuple=True)          # the threshold on the device: few pairs pass a low one
        parts.append(best_matches(names[s0:s1], seqs[s0:s1], motifs, *res, thresh=args.thresh,
                                  pairs=(si.cpu().numpy(), mi.cpu().numpy())))
    df = _merge(parts)
    write_filtered(df, f"{args.out_dir}/fimo_filtered.tsv")
    # every motif is named in fimo_out.txt: the motifs without a row add their best row of the whole run
    have = set(zip(df["motif_id"], df["motif_alt_id"]))
    extra = [m for m in range(M) if (motifs.ids[m], motifs.alt_ids[m]) not in have and int(best_s[m]) >= 0]
    rows = [df]
    for m in extra:
        s = int(best_s[m])
        res = scan(codes[s:s + 1], args.bp_pad, motifs, tables)
        rows.append(best_matches(names[s:s + 1], seqs[s:s + 1], motifs, *res, thresh=np.inf, pairs=([0], [m])))
    write_fimo_text(pd.concat(rows, ignore_index=True) if len(rows) > 1 else df, f"{args.out_dir}/fimo_out.txt")
    return df


def _merge(parts):
    """The batches' rows as one table in the order of :func:`best_matches`: p-value, sequence, motif."""
    import pandas as pd
    if not parts:
        return pd.DataFrame(columns=FIMO_COLUMNS)
    df = pd.concat(parts, ignore_index=True)[FIMO_COLUMNS]
    if len(parts) == 1:
        return df
    # batches are in sequence order and each is sorted by (p, sequence, motif): a stable sort on p restores the whole
    return df.sort_values(by="p-value", kind="stable").reset_index(drop=True)


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
