"""numpy restatement of the motif scan (expecto_amd/query_fimo_for_predictions.py, csrc/pwm.hip): the
minimal MEME parser, the strand-symmetric background, the scaled integer matrix, the score-to-p-value
table and the best match that covers a position.  Plain loops in the stated order; letters in alphabet
order A C G T except where "codes" are named (0=A 1=G 2=C 3=T, 4 and above: no base).

test_fimo_ref.py anchors it (enumeration over all 4^w sequences); test_gpu_pwm.py compares the device
with it bit for bit."""
import itertools
import re

import numpy as np

ALPHABET = "ACGT"
CODE_OF = {"A": 0, "G": 1, "C": 2, "T": 3}
LETTER_OF_CODE = "AGCT"
TO_CODE_ORDER = [0, 2, 1, 3]          # alphabet column of code 0..3
NRDB = (0.281774, 0.222020, 0.228876, 0.267330)
FIMO_COLUMNS = ['motif_id', 'motif_alt_id', 'sequence_name', 'start', 'stop', 'strand', 'score', 'p-value', 'q-value',
                'matched_sequence']


# ---- rule 1: motifs ------------------------------------------------------------------------------

def parse_meme(path):
    """-> (background [4] or None, [(id, alt, freqs [w, 4], nsites)])."""
    lines = [ln.strip() for ln in open(path)]
    bg, motifs, name, i = None, [], None, 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        if ln.startswith("Background letter frequencies"):
            tok = lines[i].split()
            i += 1
            d = dict(zip(tok[0::2], map(float, tok[1::2])))
            bg = np.array([d[a] for a in ALPHABET])
        elif ln.startswith("MOTIF"):
            tok = ln.split()
            name = (tok[1], tok[2] if len(tok) > 2 else "")
        elif ln.startswith("letter-probability matrix"):
            keys = dict(re.findall(r"(\w+)=\s*(\S+)", ln))
            if int(keys.get("alength", 4)) != 4:
                raise ValueError(name[0])
            w = int(keys["w"])
            rows = []
            while i < len(lines) and len(rows) < w:
                tok = lines[i].split()
                try:
                    row = [float(t) for t in tok]
                except ValueError:
                    break
                if len(row) != 4:
                    break
                rows.append(row)
                i += 1
            m = np.array(rows, np.float64).reshape(-1, 4)
            if len(rows) < w or (np.abs(m.sum(1) - 1) > 1e-2).any():
                raise ValueError(name[0])
            n = float(keys.get("nsites", 0))
            motifs.append((name[0], name[1], m, n if n > 0 else 20.0))
    return bg, motifs


# ---- rule 2: background --------------------------------------------------------------------------

def symmetric(bg):
    bg = np.asarray(bg, np.float64)
    at, cg = (bg[0] + bg[3]) / 2, (bg[1] + bg[2]) / 2
    return np.array([at, cg, cg, at])


# ---- rule 3: scaled matrix -----------------------------------------------------------------------

def build_pssm(freqs, nsites, bg, pseudo=0.1):
    freqs, bg = np.asarray(freqs, np.float64), np.asarray(bg, np.float64)
    f = (freqs * float(nsites) + float(pseudo) * bg) / (float(nsites) + float(pseudo))
    lo = np.log2(f / bg)
    mn, mx = float(lo.min()), float(lo.max())
    if mn == mx:
        mn = mx - 1
    scale, offset = 100 / (mx - mn), mn
    s = np.zeros(lo.shape, np.int64)
    for i in range(lo.shape[0]):
        for a in range(4):
            s[i, a] = int(np.rint((lo[i, a] - offset) * scale))
    return s, scale, offset


def raw_score(scaled_sum, w, scale, offset):
    return scaled_sum / scale + w * offset


# ---- rule 4: p-value table -----------------------------------------------------------------------

def pdf_scatter(s, bg):
    """The distribution of the scaled sum: sequential scatter, product rounded, then the add."""
    w = s.shape[0]
    b = [float(x) for x in bg]                  # Python floats are IEEE doubles: a product, then a sum, no FMA
    old = [0.0] * (100 * w + 1)
    old[0] = 1.0
    for i in range(w):
        new = [0.0] * (100 * w + 1)
        si = [int(x) for x in s[i]]
        for k in range(0, 100 * i + 1):
            for a in range(4):
                t = old[k] * b[a]
                new[k + si[a]] = new[k + si[a]] + t
        old = new
    return np.array(old, np.float64)


def pdf_gather(s, bg):
    """The same distribution gathered per target, as the kernel does: the four letters by (entry
    descending, alphabet index ascending), from +0.0; a term without a source adds +0.0."""
    w = s.shape[0]
    old = np.zeros(100 * w + 1, np.float64)
    old[0] = 1.0
    for i in range(w):
        order = sorted(range(4), key=lambda a: (-int(s[i, a]), a))
        n_old, n_new = 100 * i + 1, 100 * (i + 1) + 1
        new = np.zeros(100 * w + 1, np.float64)
        j = np.arange(n_new)
        acc = np.zeros(n_new, np.float64)
        for a in order:
            k = j - int(s[i, a])
            ok = (k >= 0) & (k < n_old)
            t = np.where(ok, old[np.clip(k, 0, n_old - 1)] * np.float64(bg[a]), 0.0)
            acc = acc + t
        new[:n_new] = acc
        old = new
    return old


def tail(pdf):
    pv = np.zeros_like(pdf)
    n = len(pdf)
    pv[n - 1] = pdf[n - 1]
    for j in range(n - 2, -1, -1):
        pv[j] = pv[j + 1] + pdf[j]
    pv = np.minimum(pv, 1.0)
    pv[0] = 1.0                 # P(score >= 0): the clip removes an excess only, and the chain can end below 1
    return pv


def pvalue_table(s, bg, gather=True):
    """s int [w, 4], bg [4], both in alphabet order -> float64 [100 w + 1]."""
    return tail(pdf_gather(s, bg) if gather else pdf_scatter(s, bg))


def pvalue_by_enumeration(s, bg):
    """pv[j] = the sum over all 4^w sequences with scaled score >= j of their probability (math.fsum)."""
    import math
    w = s.shape[0]
    by_score = [[] for _ in range(100 * w + 1)]
    for letters in itertools.product(range(4), repeat=w):
        sc = sum(int(s[i, a]) for i, a in enumerate(letters))
        by_score[sc].append(math.prod(float(bg[a]) for a in letters))
    out, terms = np.zeros(100 * w + 1), []
    for j in range(100 * w, -1, -1):
        terms += by_score[j]
        out[j] = math.fsum(terms)
    return out


# ---- rule 5: scan --------------------------------------------------------------------------------

def strand_scores(s_code, codes, p):
    """('+', '-') scaled sums of the window at p; s_code int [w, 4] in code order."""
    w = s_code.shape[0]
    plus = sum(int(s_code[i, codes[p + i]]) for i in range(w))
    minus = sum(int(s_code[w - 1 - i, 3 - codes[p + i]]) for i in range(w))
    return plus, minus


def scan_one(s_code, codes, L, c):
    """-> (score, start, strand) of the best admissible window, (-1, -1, 0) without one."""
    w = s_code.shape[0]
    best = (-1, -1, 0)
    for p in range(0, L - w + 1):
        if c >= 0 and not (p <= c <= p + w - 1):
            continue
        if any(codes[p + i] >= 4 for i in range(w)):
            continue
        plus, minus = strand_scores(s_code, codes, p)
        if plus > best[0]:
            best = (plus, p, 0)
        if minus > best[0]:
            best = (minus, p, 1)
    return best


def scan(codes, L, overlap, mats_code, tables):
    """codes uint8 [S, >= L], overlap int [S], mats_code: per motif int [w, 4] in code order, tables: per
    motif its p-value table -> score int32, start int32, strand uint8, pvalue float64, each [S, M]."""
    S, M = codes.shape[0], len(mats_code)
    score, start = np.full((S, M), -1, np.int32), np.full((S, M), -1, np.int32)
    strand, pvalue = np.zeros((S, M), np.uint8), np.full((S, M), np.nan, np.float64)
    for s in range(S):
        row = [int(x) for x in codes[s, :L]]
        for m in range(M):
            sc, p, st = scan_one(mats_code[m], row, L, int(overlap[s]))
            score[s, m], start[s, m], strand[s, m] = sc, p, st
            if sc >= 0:
                pvalue[s, m] = tables[m][sc]
    return score, start, strand, pvalue


# ---- on strings: what the command line writes ----------------------------------------------------

def revcomp(seq):
    return seq.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def codes_of(seq):
    return [CODE_OF.get(ch, 4) for ch in seq.upper()]


def filtered_rows(names, seqs, meme_motifs, bg, pad, pseudo=0.1, thresh=1.0):
    """The rows of fimo_filtered.tsv as tuples of FIMO's ten columns with the exact p-value and raw score:
    one per (motif, sequence) with a window over position ``pad`` and p <= thresh, sorted by p-value, then
    sequence, then motif.  bg: symmetric, alphabet order."""
    rows = []
    for m, (mid, alt, freqs, nsites) in enumerate(meme_motifs):
        s, scale, offset = build_pssm(freqs, nsites, bg, pseudo)
        table = pvalue_table(s, bg)
        s_code = s[:, TO_CODE_ORDER]
        w = s.shape[0]
        for v, (name, seq) in enumerate(zip(names, seqs)):
            sc, p, st = scan_one(s_code, codes_of(seq), len(seq), pad)
            if sc < 0 or not table[sc] <= thresh:
                continue
            win = seq.upper()[p:p + w]
            rows.append((table[sc], v, m, (mid, alt, name, p + 1, p + w, "+-"[st], raw_score(sc, w, scale, offset), table[sc],
                                           "", revcomp(win) if st else win)))
    rows.sort(key=lambda r: r[:3])
    return [r[3] for r in rows]


def text_row(row):
    r = list(row)
    r[6], r[7] = "%g" % r[6], "%.3g" % r[7]
    return "\t".join(str(x) for x in r)
