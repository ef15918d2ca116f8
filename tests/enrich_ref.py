"""Numpy / pure-Python restatement of the counting of the reference's ``cluster_contribs_hypergeom``
(cluster_analysis_with_fimo.py:126-162) and of the hypergeometric upper tail, for the tests of
``expecto_cluster_enrich`` and ``expecto_hypergeom_sf``: an argsort per row, Python sets, exact
integers; the tail as a Fraction of ``math.comb`` sums.  Also the recipes of the fixtures under
tests/golden/fimo (written by tests/golden/make_golden_fimo.py)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np


def order_rows(values):
    """Columns of every row by |value| descending, equal magnitudes the lower column first."""
    return np.argsort(-np.abs(np.asarray(values, np.float64)), axis=1, kind="stable")


def counts(contrib, sets, matches, sid, rows, n_neg, T, perm=None):
    """One problem.  contrib float64 [V, C]; sets: list of C Python sets of motif indices; matches: list
    of S lists of motif indices (repeats count); sid int [V] (-1: no sequence); rows: the row list;
    perm [V, C] or None: column c of row v takes contrib[v, perm[v, c]].
    Returns pos_matches [T], pos_motifs [T], neg_matches, neg_motifs (int64) and min_rank int32 [C]."""
    a = np.asarray(contrib, np.float64)
    V, C = a.shape
    if perm is not None:
        a = np.take_along_axis(a, np.asarray(perm).astype(np.int64), axis=1)
    order = order_rows(a)
    pos_matches, pos_motifs = np.zeros(T, np.int64), np.zeros(T, np.int64)
    neg_matches = neg_motifs = 0
    min_rank = np.full(C, C, np.int32)
    for v in rows:
        v = int(v)
        o = order[v]
        entries = matches[int(sid[v])] if sid[v] >= 0 else []
        for t in range(T):
            s = sets[o[t]]
            pos_matches[t] += sum(1 for m in entries if m in s)
            pos_motifs[t] += len(s)
        bottom = set().union(*[sets[c] for c in o[C - n_neg:]])
        neg_matches += sum(1 for m in entries if m in bottom)
        neg_motifs += len(bottom)
        rank = np.empty(C, np.int32)
        rank[o] = np.arange(C, dtype=np.int32)
        min_rank = np.minimum(min_rank, rank)
    return pos_matches, pos_motifs, np.int64(neg_matches), np.int64(neg_motifs), min_rank


def quadruples(pos_matches, pos_motifs, neg_matches, neg_motifs):
    """k, M, n, N of cluster_analysis_with_fimo.py:162 per top cluster index."""
    k = np.asarray(pos_matches, np.int64)
    n = np.asarray(pos_motifs, np.int64)
    return k, n + np.int64(neg_motifs), n, k + np.int64(neg_matches)


def n_unique(min_rank, T):
    return np.array([int((np.asarray(min_rank) <= t).sum()) for t in range(T)], np.int64)


def exact_sf(k, M, n, N):
    """P(X >= k) as a Fraction: the sum of comb(n, i) comb(M - n, N - i) over the tail, over comb(M, N);
    each term from the one before by an exact integer ratio.  None where scipy's argument check gives NaN."""
    k, M, n, N = int(k), int(M), int(n), int(N)
    if M <= 0 or n < 0 or N < 0 or n > M or N > M:
        return None
    lo, hi = max(0, N - (M - n)), min(n, N)
    if k <= lo:
        return Fraction(1)
    if k > hi:
        return Fraction(0)
    term = math.comb(n, k) * math.comb(M - n, N - k)
    total = term
    for i in range(k, hi):
        term = term * ((n - i) * (N - i)) // ((i + 1) * (M - n - N + i + 1))
        total += term
    return Fraction(total, math.comb(M, N))


def exact_sf_digits(k, M, n, N, digits=40):
    """:func:`exact_sf` rounded to ``digits`` significant decimal digits, as a string (None as None):
    what tests/golden/fimo/hypergeom_exact.json stores, since math.comb of a population of 1e5 and more
    takes seconds."""
    import decimal
    e = exact_sf(k, M, n, N)
    if e is None:
        return None
    if e == 0:
        return "0"
    shift = e.denominator.bit_length() - e.numerator.bit_length() + 4 * digits
    scaled = (e.numerator << shift) // e.denominator if shift >= 0 else e.numerator // (e.denominator << -shift)
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        ctx.Emin, ctx.Emax = -10 ** 7, 10 ** 7
        return str(decimal.Decimal(scaled) / (decimal.Decimal(2) ** shift))


def sf_quadruples():
    """A few hundred (k, M, n, N) for ``expecto_hypergeom_sf``: the degenerate branches, both sides of
    the mode, tails down to about 1e-300, N up to 1e5."""
    rng = np.random.RandomState(5)
    q = [(0, 10, 5, 5), (6, 10, 5, 5), (1, 10, 8, 5), (3, 10, 8, 5), (4, 10, 8, 5), (5, 10, 8, 5), (1, 1, 1, 1),
         (0, 1, 0, 0), (1, 1, 0, 1), (1, 0, 0, 0), (0, 0, 0, 0), (3, 10, 12, 5), (3, 10, 5, 12), (2, 10, -1, 5),
         (700, 5000, 1000, 1000), (660, 5000, 1000, 1000), (655, 5000, 1000, 1000), (640, 5000, 1000, 1000),
         (200, 5000, 1000, 1000), (100, 5000, 1000, 1000), (1, 5000, 1000, 1000),
         (16000, 30000, 20000, 22000), (16080, 30000, 20000, 22000), (14000, 30000, 20000, 22000),
         (560, 200000, 1000, 100000), (450, 200000, 1000, 100000), (990, 200000, 1000, 100000),
         (50500, 400000, 200000, 100000), (49000, 400000, 200000, 100000),
         (30, 1000000, 100, 100000), (1, 1000000, 100, 100000), (100, 1000000, 100, 100000)]
    for _ in range(270):
        M = int(rng.choice([20, 75, 400, 2200, 30000]))
        n, N = int(rng.randint(0, M + 1)), int(rng.randint(0, M + 1))
        lo, hi = max(0, N - (M - n)), min(n, N)
        q.append((int(rng.randint(lo - 1, hi + 3)), M, n, N))
    return q


def counts_batch(contrib, set_bits, M, seq_ptr, motif_idx, batch, n_neg, T, device=None, timings=None):
    """``cluster_analysis_with_fimo.device_counts`` by :func:`counts`: the same arguments and results."""
    set_bits = np.asarray(set_bits, np.uint64)
    sets = [{m for m in range(M) if (int(set_bits[c, m >> 6]) >> (m & 63)) & 1} for c in range(set_bits.shape[0])]
    matches = [[int(m) for m in motif_idx[seq_ptr[s]:seq_ptr[s + 1]]] for s in range(len(seq_ptr) - 1)]
    out = [[], [], [], []]
    for slot, sid_slot, off, cnt in np.asarray(batch.table).tolist():
        r = counts(contrib, sets, matches, batch.sids[sid_slot], batch.rows[off:off + cnt], n_neg, T,
                   perm=batch.perms[slot] if slot >= 0 else None)
        out[0].append(r[0]); out[1].append(r[1]); out[2].append([r[2], r[3]]); out[3].append(r[4])
    return (np.array(out[0], np.int64).reshape(-1, T), np.array(out[1], np.int64).reshape(-1, T),
            np.array(out[2], np.int64).reshape(-1, 2), np.array(out[3], np.int32).reshape(-1, set_bits.shape[0]))


def bitsets(sets, M):
    """uint64 [C, ceil(M / 64)] of the sets."""
    W = (M + 63) // 64
    out = np.zeros((len(sets), W), np.uint64)
    for c, s in enumerate(sets):
        for m in s:
            out[c, m >> 6] |= np.uint64(1) << np.uint64(m & 63)
    return out


def csr(matches):
    ptr = np.zeros(len(matches) + 1, np.int64)
    ptr[1:] = np.cumsum([len(m) for m in matches])
    idx = np.array([m for row in matches for m in row], np.int32)
    return ptr, idx


# ---- fixtures of tests/golden/fimo ---------------------------------------------------------------

N_NEG = 20                                 # the reference's keyword default
GENES = ("ENSG_A", "ENSG_B", "ENSG_C", "ENSG_D")
RSIDS = tuple(f"rs{100 + i}" for i in range(9))
ROW_RSID = (0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 3, 3)           # 12 rows over 9 rsids; rows 3, 10, 11 share one
ROW_GENE = (0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 0)
LEADING = ("0", "1", "2", "3", "4", "5", "6", "7", "dist", "gene", "strand", "REF", "ALT", "SED", "SED_PROPORTION")


def fixture(case: str):
    """The three input tables of a golden case as text: (cluster_contribs.tsv, rsat_clusters.tsv,
    fimo.tsv).  ``main``: 25 clusters of 3 motifs plus cluster_-1 (T = 6).  ``shared``: the same, but
    the first motif of cluster k also sits in cluster k+1 (one name in two clusters)."""
    assert case in ("main", "shared")
    rng = np.random.RandomState(20 if case == "main" else 21)
    C, per = 25, 3
    names = [[f"M{c:02d}{'abc'[j]}_HUMAN.H11MO.0.A" for j in range(per)] for c in range(C)]
    if case == "shared":
        for c in range(C - 1):
            names[c + 1].append(names[c][0])
    V = len(ROW_RSID)
    contrib = rng.standard_normal((V, C)) * np.exp(rng.uniform(-3, 1, (V, C)))
    mags = np.abs(contrib)
    for v in range(V):
        assert len(set(mags[v].tolist())) == C, "two equal magnitudes in a row: outside what the reference defines"
    sed = rng.standard_normal(V) * 0.01
    prop = np.abs(sed) / rng.uniform(1.0, 4.0, V)
    assert len(set(prop.tolist())) == V
    head = ["index", *LEADING, *[f"cluster_{c + 1}" for c in range(C)], "cluster_-1"]
    lines = ["\t".join(head)]
    for v in range(V):
        lead = [f"chr{1 + v % 3}", str(1000 * (v + 1)), RSIDS[ROW_RSID[v]], "A", "C", "x", "y", "z", str(17 * v - 60),
                GENES[ROW_GENE[v]], "+-"[v % 2], repr(float(1.0 + v)), repr(float(1.0 + v + sed[v])), repr(float(sed[v])),
                repr(float(prop[v]))]
        lines.append("\t".join([str(v), *lead, *[repr(float(x)) for x in contrib[v]], repr(float(rng.standard_normal()))]))
    contribs_tsv = "\n".join(lines) + "\n"

    clusters_tsv = "".join(f"cluster_{c + 1}\t{','.join(names[c])}\n" for c in range(C)) + "cluster_-1\tSTAT3,UNPLACED\n"

    motifs = sorted({m for row in names for m in row})
    fimo = ["# motif_id\tmotif_alt_id\tsequence_name\tstart\tstop\tstrand\tscore\tp-value\tq-value\tmatched_sequence"]
    k = 0

    def add(motif, seq, start, stop, p):
        nonlocal k
        fimo.append("\t".join([f"MA{k % 7:04d}.1", motif, seq, str(start), str(stop), "+-"[k % 2], f"{10 + k % 5}.5",
                               repr(float(p)), "0.5", "ACGTACGT"]))
        k += 1

    for i, m in enumerate(motifs):                       # every motif at least once (the script's assert)
        seq = RSIDS[i % 8]                               # rs108 gets no row at all
        inside = i % 5 != 0
        start = 25 + i % 6 if inside else 33 + i % 4     # the variant sits at position 31
        p = 10.0 ** -(4.5 + (i % 4)) if i % 7 else 3e-4  # some above the 1e-4 threshold
        add(m, seq, start, start + 9, p)
    for j in range(60):                                  # more rows: repeats of a motif in a sequence, other ids
        m = motifs[int(rng.randint(len(motifs)))]
        seq = RSIDS[int(rng.randint(8))]
        start = int(rng.randint(18, 36))
        add(m, seq, start, start + int(rng.randint(6, 14)), 10.0 ** -rng.uniform(3.5, 8.0))
    add(motifs[0], "rs_elsewhere", 28, 36, 1e-6)         # a sequence no row names
    fimo_tsv = "\n".join(fimo) + "\n"
    return contribs_tsv, clusters_tsv, fimo_tsv
