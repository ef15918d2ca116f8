"""Drop-in for the reference ``cluster_analysis_with_fimo.py``: are the motif clusters that drive a
variant's predicted effect (``cluster_contribs.tsv`` / ``rsat_clusters.tsv`` of
``expecto_amd.predict_by_cluster --rsat_clusters_tab``) the clusters whose motifs match the sequence at
the variant (a FIMO text table)?  One hypergeometric p-value per "top cluster index".

    python -m expecto_amd.cluster_analysis_with_fimo --cluster_contribs_file cluster_contribs.tsv \\
        --rsat_clusters_file rsat_clusters.tsv --fimo_out_file fimo.tsv [--rank_int] [--upstream_bp 30] \\
        [--downstream_bp 30] [--pval_match_threshold 1e-4] [--n_neg_clusters 20] [--n_permutations 1] \\
        [-o temp_cluster_analysis_with_fimo]

Without a FIMO table: ``--motif_file M.meme --vcf_file V [--hg19_fasta F] [--bgfile nrdb] [--motif-pseudo 0.1]
[--seq-batch 8192]`` in place of ``--fimo_out_file`` scans the motifs over the variants' flanks on the device
(``expecto_amd.query_fimo_for_predictions``: :func:`scan_matches`); the matches never become text.

Reading and filtering are the reference's pandas calls (cluster_analysis_with_fimo.py:31-58).  The
triple loop of ``cluster_contribs_hypergeom`` is ``expecto_cluster_enrich`` (include/expecto_hip.h): the
seven problems of a run (the data, shuffled clusters, shuffled variants, four SED quartiles) are one
call, their p-values one ``expecto_hypergeom_sf`` call.  The shuffles are drawn on the host from
``RandomState(1)`` with the reference's calls in the reference's order (:func:`draw_shuffles`), so the
two shuffled problems are the reference's.  ``--n_permutations P`` continues that stream: permutation
``j >= 1`` draws ``rand(V, C).argsort(1)`` and then ``choice(V, V, replace=False)``; they go to the device
in chunks of :func:`chunk_size` permutations.  Stdout is the reference's.

Differences from the reference, on purpose:
* the cluster columns are those from the first column named ``cluster_*`` on, not from position 15
  (the reference assumes an 8-column VCF; ours has 5);
* ``--n_neg_clusters`` (a keyword default there), ``--n_permutations``; the numeric arguments are parsed
  as numbers;
* equal magnitudes in a row take the lower column first (pandas' sort is not stable there);
* ``T > C`` (an IndexError there) and a cluster column missing from the cluster table (a KeyError) are
  ``ValueError``s that say why;
* no PDFs: ``hypergeom.tsv``, ``num_unique_clusters.tsv`` and, with ``P > 1``, ``permutation_null.tsv``.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import NamedTuple

import numpy as np

MAX_C, MAX_M = 1024, 32768                 # include/expecto_hip.h
PERM_BYTES = 256 << 20                     # host / device bytes of permutations per chunk
CONTROLS = ("shuffled_clusters", "shuffled_variants")
PERCENTILES = tuple((x, x + 25) for x in range(0, 100, 25))
PROBLEMS = ("top", *CONTROLS, *[f"percentile_{a}_{b}" for a, b in PERCENTILES])
FIMO_COLUMNS = ['motif_id', 'motif_alt_id', 'sequence_name', 'start', 'stop', 'strand', 'score', 'p-value', 'q-value',
                'matched_sequence']


class Inputs(NamedTuple):
    contrib: np.ndarray        # float64 [V, C]: the cluster columns without cluster_-1
    columns: list              # their names
    sets: list                 # per column the set of its motif indices
    motifs: list               # motif names; the index is the motif's bit
    matches: object            # per sequence the motif indices of its filtered FIMO rows (--motif_file: their CSR pair)
    sequences: list            # distinct FIMO sequence names (--motif_file: the variants' IDs)
    sid: np.ndarray            # int32 [V]: the row's sequence, -1 without one
    sed: np.ndarray            # float64 [V]: the column the quartiles are cut on
    n_cluster_rows: int        # rows of the cluster table, cluster_-1 among them


class Batch(NamedTuple):
    """Problems of one ``expecto_cluster_enrich`` call."""
    table: np.ndarray          # int64 [P, 4]: permutation slot (-1: none), sid slot, row offset, row count
    perms: np.ndarray          # uint16 [n_perms, V, C]
    sids: np.ndarray           # int32 [n_sids, V]
    rows: np.ndarray           # int32 [rows_len]


class Enrichment(NamedTuple):
    pos_matches: np.ndarray    # int64 [P, T]
    pos_motifs: np.ndarray     # int64 [P, T]
    neg_matches: np.ndarray    # int64 [P]
    neg_motifs: np.ndarray     # int64 [P]
    min_rank: np.ndarray       # int32 [P, C]
    k: np.ndarray              # int64 [P, T] each: the quadruple of hypergeom.sf(k - 1, M, n, N)
    M: np.ndarray
    n: np.ndarray
    N: np.ndarray
    pval: np.ndarray           # float64 [P, T]

    def n_unique(self, p=0):
        """Distinct columns among the first t + 1 ranks of any row, for t < T."""
        T = self.pos_matches.shape[1]
        return np.array([int((self.min_rank[p] <= t).sum()) for t in range(T)], np.int64)


# ---- reading (cluster_analysis_with_fimo.py:31-58) --------------------------------------------

def rank_int(sed, genes, rs, c=3.0 / 8):
    """``groupby("gene")["SED"].transform(rank_INT, stochastic=True)``: per gene, in sorted gene order,
    ``seed(123)``, a permutation of the gene's rows, ordinal ranks in that order, ``norm.ppf`` of
    ``(rank - c) / (n - 2c + 1)``.  Every call reseeds ``rs``: the shuffles that follow read the stream
    the last gene left."""
    from scipy.stats import norm, rankdata

    sed = np.asarray(sed, np.float64)
    if np.isnan(sed).any():
        raise ValueError("--rank_int: NaN in the SED column")
    genes = np.asarray(genes)
    out = np.empty(len(sed), np.float64)
    for g in sorted(set(genes.tolist())):
        labels = np.nonzero(genes == g)[0]
        rs.seed(123)
        labels = rs.permutation(labels)
        rank = rankdata(sed[labels], method="ordinal")
        out[labels] = norm.ppf((rank - c) / (len(rank) - 2 * c + 1))
    return out


def load(args, rs=None) -> Inputs:
    """The three tables, filtered as the reference filters them.  ``rs``: the run's RandomState, moved
    by ``--rank_int`` only."""
    import pandas as pd

    rsat_clusters_df = pd.read_csv(args.rsat_clusters_file, sep="\t", header=None, index_col=0)
    cluster_contribs_df = pd.read_csv(args.cluster_contribs_file, sep="\t", index_col=0).drop("cluster_-1", axis=1) \
                                                                                        .reset_index(drop=True)
    names = [str(c) for c in cluster_contribs_df.columns]
    first = next((i for i, c in enumerate(names) if c.startswith("cluster_")), None)
    if first is None:
        raise ValueError(f"{args.cluster_contribs_file}: no column named cluster_*")
    columns = names[first:]
    contrib = np.ascontiguousarray(cluster_contribs_df.iloc[:, first:].to_numpy(np.float64))
    if "2" not in names[:first]:
        raise ValueError(f"{args.cluster_contribs_file}: no column labelled 2 (the rsid) before the cluster columns")
    rsids = cluster_contribs_df["2"].tolist()

    sed = cluster_contribs_df["SED" if args.rank_int else "SED_PROPORTION"].to_numpy(np.float64)
    if args.rank_int:
        sed = rank_int(sed, cluster_contribs_df["gene"].to_numpy(), rs if rs is not None else np.random.RandomState(1))

    per_cluster = {str(k): str(v).split(",") for k, v in rsat_clusters_df[1].items()}
    placed = set(sum(rsat_clusters_df[1][:-1].str.split(",").tolist(), []))          # skip cluster_-1
    missing = [c for c in columns if c not in per_cluster]
    motifs = sorted(set(sum(per_cluster.values(), [])))
    bit = {m: i for i, m in enumerate(motifs)}
    sets = None if missing else [{bit[m] for m in per_cluster[c]} for c in columns]

    def agree(source, n_motifs_total):
        if n_motifs_total != len(placed):
            raise ValueError(f"{source} names {n_motifs_total} motifs, the clusters of "
                             f"{args.rsat_clusters_file} hold {len(placed)} (the reference asserts that they agree)")
        if missing:
            raise ValueError(f"{args.rsat_clusters_file} has no row for {missing[0]} "
                             f"(and {len(missing) - 1} more columns of {args.cluster_contribs_file})")

    if getattr(args, "fimo_out_file", None) is None:
        matches, sequences, sid = scan_matches(args, bit, rsids, agree)
        return Inputs(contrib, columns, sets, motifs, matches, sequences, sid, sed, int(rsat_clusters_df.shape[0]))

    fimo_df = pd.read_table(args.fimo_out_file, sep='\t', names=FIMO_COLUMNS, comment='#')
    agree(args.fimo_out_file, len(set(fimo_df["motif_alt_id"])))

    # subset to motifs within range of the variant, the most significant match per motif and variant, threshold
    fimo_df = fimo_df[(fimo_df["start"] <= (args.upstream_bp + 1)) & (fimo_df["stop"] >= (args.upstream_bp + 1))]
    fimo_df = fimo_df.sort_values(by="p-value").drop_duplicates(subset=["motif_id", "motif_alt_id", "sequence_name"],
                                                                keep="first")
    fimo_df = fimo_df[fimo_df["p-value"] < args.pval_match_threshold]

    sequences, where, matches = [], {}, []
    for name, motif in zip(fimo_df["sequence_name"].tolist(), fimo_df["motif_alt_id"].tolist()):
        if name not in where:
            where[name] = len(sequences)
            sequences.append(name)
            matches.append([])
        if motif in bit:
            matches[where[name]].append(bit[motif])
    sid = np.array([where.get(r, -1) for r in rsids], np.int32)
    return Inputs(contrib, columns, sets, motifs, matches, sequences, sid, sed, int(rsat_clusters_df.shape[0]))


def scan_matches(args, bit, rsids, agree):
    """The ``--motif_file`` route: the motifs of a MEME file scanned on the device over the flanks
    ``POS - upstream_bp .. POS + downstream_bp`` of the variants of ``--vcf_file``
    (query_fimo_for_predictions: ``scan`` + ``matches_csr``); no FIMO table.  A match is the best window
    over the variant with p < ``--pval_match_threshold``, the filter of the other route.  Returns the CSR
    pair of the matches in ``bit`` numbering, the sequence names and the rows' sequences."""
    from . import query_fimo_for_predictions as q
    from .genome import open_genome

    meme = q.read_meme(args.motif_file)
    agree(args.motif_file, len(set(meme.alt_ids)))
    bg = q.background(args.bgfile, meme)
    motifs = q.Motifs.from_meme(meme, bg, args.motif_pseudo)
    names, _, codes = q.flanks(q.read_vcf(args.vcf_file), open_genome(args.hg19_fasta), args.upstream_bp,
                               args.downstream_bp)
    where = {n: i for i, n in enumerate(names)}
    if len(where) != len(names):
        raise ValueError(f"{args.vcf_file}: a variant ID appears twice; the rows of {args.cluster_contribs_file} find "
                         "their sequence by it")
    tables = q.pvalue_tables(motifs, bg)
    motif_map = np.array([bit.get(a, -1) for a in motifs.alt_ids], np.int64)
    ptrs, idxs = [np.zeros(1, np.int64)], [np.zeros(0, np.int32)]
    for s0 in range(0, len(names), max(1, args.seq_batch)):
        res = q.scan(codes[s0:s0 + max(1, args.seq_batch)], args.upstream_bp, motifs, tables)
        ptr, idx = q.matches_csr(res[3], args.pval_match_threshold, motif_map)
        ptrs.append(ptr[1:] + ptrs[-1][-1])
        idxs.append(idx)
    sid = np.array([where.get(r, -1) for r in rsids], np.int32)
    return (np.concatenate(ptrs), np.concatenate(idxs).astype(np.int32)), names, sid


# ---- problems ---------------------------------------------------------------------------------

def draw_shuffles(rs, V: int, C: int, P: int):
    """Yield ``(idx uint16 [V, C], random_idxs int64 [V])`` for permutation 0 .. P-1 from ``rs``, each with
    the reference's two calls in the reference's order: ``rand(V, C).argsort(1)``
    (shuffle_along_axis), then ``choice(V, V, replace=False)``.  Shuffled clusters: column c of row v
    takes ``contrib[v, idx[v, c]]``; shuffled variants: row v takes the rsid of row ``random_idxs[v]``."""
    for _ in range(int(P)):
        idx = rs.rand(V, C).argsort(axis=1).astype(np.uint16)
        yield idx, rs.choice(V, V, replace=False)


def quartile_rows(sed):
    """Per percentile range the rows with ``lower <= sed <= upper`` (both ends: neighbours share a row)."""
    out = []
    for a, b in PERCENTILES:
        lower, upper = np.percentile(sed, a), np.percentile(sed, b)
        out.append(np.nonzero((lower <= sed) & (sed <= upper))[0].astype(np.int32))
    return out


def reference_batch(inp: Inputs, idx, random_idxs) -> Batch:
    """The seven problems of the reference, in its order (``PROBLEMS``)."""
    V = inp.contrib.shape[0]
    every = np.arange(V, dtype=np.int32)
    lists = [every] + quartile_rows(inp.sed)
    off = np.concatenate([[0], np.cumsum([len(r) for r in lists])])
    table = [(-1, 0, 0, V), (0, 0, 0, V), (-1, 1, 0, V)] + [(-1, 0, off[q + 1], len(lists[q + 1])) for q in range(4)]
    sids = np.stack([inp.sid, inp.sid[np.asarray(random_idxs)]]).astype(np.int32)
    return Batch(np.array(table, np.int64), np.ascontiguousarray(idx, np.uint16)[None], sids,
                 np.concatenate(lists).astype(np.int32))


def permutation_batch(inp: Inputs, draws) -> Batch:
    """Further permutations ``draws`` = [(idx, random_idxs)]: a shuffled-clusters and a shuffled-variants
    problem each, in that order (problem 2j and 2j + 1)."""
    V = inp.contrib.shape[0]
    table = []
    for j in range(len(draws)):
        table += [(j, 0, 0, V), (-1, 1 + j, 0, V)]
    sids = np.stack([inp.sid] + [inp.sid[np.asarray(r)] for _, r in draws]).astype(np.int32)
    return Batch(np.array(table, np.int64), np.stack([i for i, _ in draws]).astype(np.uint16), sids,
                 np.arange(V, dtype=np.int32))


def chunk_size(V: int, C: int, budget: int = PERM_BYTES) -> int:
    """Permutations per device call: what ``budget`` bytes of uint16 [V, C] and int32 [V] hold, at least 1."""
    return max(1, int(budget) // max(1, 2 * V * C + 4 * V))


# ---- device -----------------------------------------------------------------------------------

def bitsets(sets, M: int) -> np.ndarray:
    """uint64 [C, ceil(M / 64)]: bit m of row c is set when motif m is in set c."""
    out = np.zeros((len(sets), (M + 63) // 64), np.uint64)
    for c, s in enumerate(sets):
        for m in s:
            if not 0 <= m < M:
                raise ValueError(f"motif index {m} of set {c} outside [0, {M})")
            out[c, m >> 6] |= np.uint64(1) << np.uint64(m & 63)
    return out


def csr(matches):
    ptr = np.zeros(len(matches) + 1, np.int64)
    ptr[1:] = np.cumsum([len(m) for m in matches])
    flat = [m for row in matches for m in row]
    return ptr, np.array(flat, np.int32).reshape(-1)


def device_counts(contrib, set_bits, M, seq_ptr, motif_idx, batch: Batch, n_neg, T, device=None, timings=None):
    """One ``expecto_cluster_enrich`` call.  ``contrib``: float64 [V, C] on the host, or a float64 device
    tensor [V, >= C] with unit column stride (used in place).  Returns pos_matches [P, T], pos_motifs
    [P, T], neg [P, 2] (int64) and min_rank int32 [P, C].  ``timings`` adds ``upload_ms`` (host clock
    around the copies, synchronised) and ``enrich_ms`` (device events)."""
    from . import _lib
    torch = _lib.require_gpu("cluster_analysis_with_fimo")
    lib = _lib.load()
    C = int(set_bits.shape[0])
    P = int(batch.table.shape[0])
    S = len(seq_ptr) - 1
    if torch.is_tensor(contrib):
        if not contrib.is_cuda or contrib.dtype != torch.float64 or contrib.dim() != 2 or contrib.stride(1) != 1:
            raise ValueError("contrib tensor must be float64 [V, >= C] on the device with contiguous rows")
        dev = contrib.device
        V, ld = int(contrib.shape[0]), int(contrib.stride(0)) if contrib.shape[0] > 1 else int(contrib.shape[1])
    else:
        contrib = np.ascontiguousarray(contrib, np.float64)
        dev = _lib.device_of(device)
        V, ld = contrib.shape
    empty = (np.zeros((P, T), np.int64), np.zeros((P, T), np.int64), np.zeros((P, 2), np.int64),
             np.full((P, C), C, np.int32))
    if P == 0 or V == 0:
        return empty
    table = np.ascontiguousarray(batch.table, np.int64)
    seq_ptr = np.ascontiguousarray(seq_ptr, np.int64)
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        up = lambda a: _lib.upload(a, dev)
        cd = contrib if torch.is_tensor(contrib) else up(contrib)
        bits_d, ptr_d, idx_d, tab_d = up(set_bits.view(np.int64)), up(seq_ptr), up(motif_idx), up(table)
        perms_d, sids_d, rows_d = up(batch.perms.view(np.int16)), up(batch.sids), up(batch.rows)
        nbytes = int(lib.expecto_cluster_enrich_workspace(S, C))
        ws = _lib.workspace(max(nbytes, 4), dev)
        pos_m = torch.empty((P, T), dtype=torch.int64, device=dev)
        pos_b = torch.empty((P, T), dtype=torch.int64, device=dev)
        neg = torch.empty((P, 2), dtype=torch.int64, device=dev)
        min_rank = torch.empty((P, C), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        timer = _lib.EventTimer(timings)
        timer.mark()
        _lib.call("expecto_cluster_enrich", cd.data_ptr(), V, C, ld, bits_d.data_ptr(), int(M), seq_ptr.ctypes.data,
                  ptr_d.data_ptr(), idx_d.data_ptr() if idx_d.numel() else None, S, table.ctypes.data,
                  tab_d.data_ptr(), P, perms_d.data_ptr() if perms_d.numel() else None, int(batch.perms.shape[0]),
                  sids_d.data_ptr(), int(batch.sids.shape[0]), rows_d.data_ptr(), int(batch.rows.shape[0]),
                  int(n_neg), int(T), pos_m.data_ptr(), pos_b.data_ptr(), neg.data_ptr(), min_rank.data_ptr(),
                  ws.data_ptr(), max(nbytes, 4))
        timer.mark()
        out = (pos_m.cpu().numpy(), pos_b.cpu().numpy(), neg.cpu().numpy(), min_rank.cpu().numpy())
        if timings is not None:
            timings["upload_ms"] = timings.get("upload_ms", 0.0) + 1e3 * (t1 - t0)
        timer.add("enrich_ms")
    return out


def device_sf(k, M, n, N, device=None, timings=None):
    """``scipy.stats.hypergeom.sf(k - 1, M, n, N)`` of int64 arrays of one shape, by one
    ``expecto_hypergeom_sf`` call.  ``timings`` adds ``sf_ms`` (device events)."""
    from . import _lib
    torch = _lib.require_gpu("cluster_analysis_with_fimo")
    k = np.ascontiguousarray(k, np.int64)
    dev = _lib.device_of(device)
    if k.size == 0:
        return np.zeros(k.shape, np.float64)
    with torch.cuda.device(dev):
        q = _lib.upload(np.stack([k.ravel()] + [np.ascontiguousarray(a, np.int64).ravel() for a in (M, n, N)]), dev)
        out = torch.empty(k.size, dtype=torch.float64, device=dev)
        timer = _lib.EventTimer(timings)
        timer.mark()
        _lib.call("expecto_hypergeom_sf", q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), q[3].data_ptr(), k.size,
                  out.data_ptr())
        timer.mark()
        res = out.cpu().numpy().reshape(k.shape)
        timer.add("sf_ms")
    return res


def enrichment(contribs, cluster_sets, matches, batch: Batch, n_neg: int, T: int, n_motifs=None, device=None,
               timings=None) -> Enrichment:
    """Counts and p-values of the problems of ``batch``.

    contribs: float64 [V, C] (host array, or a device tensor used in place).  cluster_sets: the C motif
    sets, as Python sets of motif indices (then ``n_motifs`` is the number of motifs) or as the uint64
    bitsets [C, ceil(n_motifs / 64)].  matches: per sequence the list of motif indices, or the CSR pair
    ``(seq_ptr int64 [S + 1], motif_idx int32)``.  ``ValueError`` for what the kernel refuses (C, M,
    n_neg, T, NaN), before the device is touched where the data are on the host."""
    if isinstance(cluster_sets, np.ndarray):
        set_bits = np.ascontiguousarray(cluster_sets, np.uint64)
        M = int(n_motifs) if n_motifs is not None else 64 * set_bits.shape[1]
    else:
        M = int(n_motifs) if n_motifs is not None else 1 + max([m for s in cluster_sets for m in s], default=0)
        set_bits = bitsets(cluster_sets, M)
    C = int(set_bits.shape[0])
    if not 1 <= C <= MAX_C:
        raise ValueError(f"enrichment: {C} cluster columns; supported are 1..{MAX_C}")
    if not 1 <= M <= MAX_M:
        raise ValueError(f"enrichment: {M} motifs; supported are 1..{MAX_M}")
    if not 1 <= int(n_neg) <= C:
        raise ValueError(f"enrichment: n_neg = {n_neg} outside [1, C = {C}]")
    if not 1 <= int(T) <= C:
        raise ValueError(f"enrichment: T = {T} outside [1, C = {C}]")
    if not hasattr(contribs, "is_cuda"):
        contribs = np.ascontiguousarray(contribs, np.float64)
        if contribs.ndim != 2 or contribs.shape[1] != C:
            raise ValueError(f"enrichment: contribs has shape {contribs.shape}, the sets give C = {C}")
        if np.isnan(contribs).any():
            raise ValueError("enrichment: NaN in contribs")
    seq_ptr, motif_idx = matches if isinstance(matches, tuple) else csr(matches)
    pos_m, pos_b, neg, min_rank = device_counts(contribs, set_bits, M, seq_ptr, motif_idx, batch, n_neg, T,
                                                device=device, timings=timings)
    k, n = pos_m, pos_b
    Mq, Nq = n + neg[:, 1:2], k + neg[:, 0:1]
    pval = device_sf(k, Mq, n, Nq, device=device, timings=timings)
    return Enrichment(pos_m, pos_b, neg[:, 0].copy(), neg[:, 1].copy(), min_rank, k, Mq, n, Nq, pval)


# ---- CLI --------------------------------------------------------------------------------------

def build_parser():
    """The arguments of cluster_analysis_with_fimo.py:14-24, the numeric ones parsed as numbers, and the
    two the reference has as constants."""
    parser = argparse.ArgumentParser(prog="python -m expecto_amd.cluster_analysis_with_fimo",
                                     description='Analyze fimo results with cluster contribs')
    parser.add_argument("--cluster_contribs_file", required=True)
    parser.add_argument("--rsat_clusters_file", required=True)
    parser.add_argument("--fimo_out_file", default=None, help="a FIMO text table; or give --motif_file and --vcf_file")
    parser.add_argument("--motif_file", default=None, help="a MEME file: its motifs are scanned on the device")
    parser.add_argument("--vcf_file", default=None, help="with --motif_file: the variants")
    parser.add_argument("--hg19_fasta", default="resources/hg19.fa")
    parser.add_argument("--bgfile", default="nrdb", help="nrdb, motif-file, uniform, or a file of 'A 0.29' lines")
    parser.add_argument("--motif-pseudo", dest="motif_pseudo", type=float, default=0.1)
    parser.add_argument("--seq-batch", dest="seq_batch", type=int, default=8192, help="sequences per device call")
    parser.add_argument("--rank_int", default=False, action="store_true",
                        help="use rank-based inverse normal transformation for SED scores")
    parser.add_argument("--upstream_bp", type=int, default=30)
    parser.add_argument("--downstream_bp", type=int, default=30)
    parser.add_argument("--pval_match_threshold", type=float, default=1e-4)
    parser.add_argument("--n_neg_clusters", type=int, default=20,
                        help="the bottom clusters of a variant that form the comparison set")
    parser.add_argument("--n_permutations", type=int, default=1,
                        help="shuffles per control; above 1 also writes permutation_null.tsv")
    parser.add_argument('-o', dest="out_dir", type=str, default='temp_cluster_analysis_with_fimo', help='Output directory')
    return parser


def null_summary(observed, null):
    """Per index: median, 5th and 95th percentile of the null's -log10 p, and the empirical p-value
    (1 + #{null p <= observed p}) / (1 + P).  observed [T], null [P, T]."""
    with np.errstate(divide="ignore"):
        logs = -np.log10(null)
    emp = (1.0 + (null <= observed[None, :]).sum(axis=0)) / (1.0 + null.shape[0])
    return np.median(logs, axis=0), np.percentile(logs, 5, axis=0), np.percentile(logs, 95, axis=0), emp


def run(args, out=None, timings=None):
    """One CLI run; returns ``(Enrichment of the seven problems, null p-values [2, P, T] or None)``."""
    out = out if out is not None else sys.stdout
    if args.n_neg_clusters < 1:
        raise ValueError("--n_neg_clusters must be at least 1")
    if args.n_permutations < 1:
        raise ValueError("--n_permutations must be at least 1")
    if route_error(args):
        raise ValueError(route_error(args))
    os.makedirs(args.out_dir, exist_ok=True)
    rs = np.random.RandomState(1)
    inp = load(args, rs)
    V, C = inp.contrib.shape
    T = inp.n_cluster_rows - args.n_neg_clusters
    if T > C:
        raise ValueError(f"{inp.n_cluster_rows} rows of {args.rsat_clusters_file} less --n_neg_clusters "
                         f"{args.n_neg_clusters} leave {T} top cluster indices, {args.cluster_contribs_file} has "
                         f"only {C} cluster columns")
    n_neg = min(args.n_neg_clusters, C)          # index[-n_neg:] of C columns: all of them when n_neg > C
    P = args.n_permutations
    t0 = time.perf_counter()
    shuffles = draw_shuffles(rs, V, C, P)
    first = next(shuffles)
    draw_s = time.perf_counter() - t0
    set_bits = bitsets(inp.sets, len(inp.motifs))
    match_csr = inp.matches if isinstance(inp.matches, tuple) else csr(inp.matches)

    null = None
    if T >= 1 and V >= 1:
        res = enrichment(inp.contrib, set_bits, match_csr, reference_batch(inp, *first), n_neg, T,
                         n_motifs=len(inp.motifs), timings=timings)
        if P > 1:
            null = np.empty((2, P, T), np.float64)
            null[:, 0] = res.pval[1:3]
            step = chunk_size(V, C)
            for j0 in range(1, P, step):
                t0 = time.perf_counter()
                draws = [next(shuffles) for _ in range(min(step, P - j0))]
                draw_s += time.perf_counter() - t0
                part = enrichment(inp.contrib, set_bits, match_csr, permutation_batch(inp, draws), n_neg, T,
                                  n_motifs=len(inp.motifs), timings=timings)
                null[0, j0:j0 + len(draws)] = part.pval[0::2]
                null[1, j0:j0 + len(draws)] = part.pval[1::2]
    else:
        z = np.zeros((len(PROBLEMS), 0), np.int64)
        res = Enrichment(z, z, z[:, 0], z[:, 0], np.full((len(PROBLEMS), C), C, np.int32), z, z, z, z,
                         np.zeros((len(PROBLEMS), 0), np.float64))
        T = 0
    if timings is not None:
        timings["draw_ms"] = 1e3 * draw_s

    for p in range(len(PROBLEMS)):
        for t in range(T):
            print(f"Top cluster index: {t}, hypergeometric pval: {float(res.pval[p, t])}", file=out)
    with open(f"{args.out_dir}/hypergeom.tsv", "w") as f:
        f.write("problem\ttop_cluster_idx\tk\tM\tn\tN\thypergeom_pval\n")
        for p, name in enumerate(PROBLEMS):
            f.writelines(f"{name}\t{t}\t{res.k[p, t]}\t{res.M[p, t]}\t{res.n[p, t]}\t{res.N[p, t]}\t"
                         f"{float(res.pval[p, t])!r}\n" for t in range(T))
    with open(f"{args.out_dir}/num_unique_clusters.tsv", "w") as f:
        f.write("top_cluster_idx\tn_unique_clusters\n")
        f.writelines(f"{t}\t{u}\n" for t, u in enumerate(res.n_unique(0)))
    if null is not None:
        with open(f"{args.out_dir}/permutation_null.tsv", "w") as f:
            f.write("control\ttop_cluster_idx\tobserved_pval\tnull_median_neg_log10_pval\tnull_p05_neg_log10_pval\t"
                    "null_p95_neg_log10_pval\tempirical_pval\n")
            for c, name in enumerate(CONTROLS):
                med, p05, p95, emp = null_summary(res.pval[0], null[c])
                f.writelines(f"{name}\t{t}\t{float(res.pval[0, t])!r}\t{float(med[t])!r}\t{float(p05[t])!r}\t"
                             f"{float(p95[t])!r}\t{float(emp[t])!r}\n" for t in range(T))
    print("end", file=out)
    return res, null


def route_error(args):
    """Why the arguments name no single source of matches, or None."""
    table, scan = getattr(args, "fimo_out_file", None), getattr(args, "motif_file", None)
    if table is not None and scan is not None:
        return "give --fimo_out_file or --motif_file, not both"
    if table is None and scan is None:
        return "give --fimo_out_file, or --motif_file with --vcf_file"
    if scan is not None and getattr(args, "vcf_file", None) is None:
        return "--motif_file needs --vcf_file"
    return None


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if route_error(args):
        parser.error(route_error(args))
    return run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
