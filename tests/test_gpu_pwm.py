"""``expecto_pwm_pvalues`` and ``expecto_pwm_scan`` on the device (csrc/pwm.hip), through their C entry points,
``expecto_amd.query_fimo_for_predictions`` and the two command lines.

Outputs lie in pattern-filled buffers (tests/guarded.py), the p-value tables back to back in a buffer of
exactly their size, the sequence codes inside margins of code 4 with other codes in the row padding.
Everything is compared bitwise with the restatement (tests/fimo_ref.py), which test_fimo_ref.py anchors.
The scan kernel takes 64 sequences x 16 motifs per workgroup; the p-value kernel one motif."""
import functools
import io

import numpy as np
import pandas as pd
import pytest
import torch

import fimo_ref
from guarded import Guarded, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

BG = fimo_ref.symmetric(fimo_ref.NRDB)                     # alphabet order
BG_CODE = np.ascontiguousarray(BG[fimo_ref.TO_CODE_ORDER])
SEQ_TILE, MOTIF_TILE = 64, 16


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def q():
    from expecto_amd import query_fimo_for_predictions
    return query_fimo_for_predictions


@functools.lru_cache(maxsize=None)
def motif(w, seed=0, flat=False):
    """Scaled matrix int64 [w, 4] in code order; ``flat``: four equal entries in every column."""
    rng = np.random.RandomState(7919 * w + seed)
    if flat:
        m = np.repeat(rng.randint(0, 101, (w, 1)), 4, axis=1).astype(np.int64)
    else:
        m = rng.randint(0, 101, (w, 4)).astype(np.int64)
        m[rng.randint(0, w), rng.randint(0, 4)] = 100
        m[rng.randint(0, w), rng.randint(0, 4)] = 0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ref_table(w, seed=0, flat=False):
    t = fimo_ref.pvalue_table(motif(w, seed, flat)[:, fimo_ref.TO_CODE_ORDER], BG, gather=False)
    t.setflags(write=False)
    return t


def pack(mats):
    col_ptr = np.zeros(len(mats) + 1, np.int32)
    col_ptr[1:] = np.cumsum([m.shape[0] for m in mats])
    pssm = np.concatenate(mats).astype(np.int16) if mats else np.zeros((0, 4), np.int16)
    return np.ascontiguousarray(pssm), col_ptr


def pvalues_device(lib, pssm, col_ptr, status=0):
    """The entry point on guarded outputs -> (tables, pv_ptr), or the message of the refusal expected."""
    M = len(col_ptr) - 1
    n = max(1, 100 * int(max(col_ptr[-1], 0)) + M)
    tables, pv_ptr = Guarded((n,), np.float64), Guarded((M + 1,), np.int64)
    d_pssm, d_ptr = dev(pssm) if pssm.size else None, dev(col_ptr)
    st = lib.expecto_pwm_pvalues(d_pssm.data_ptr() if pssm.size else None, col_ptr.ctypes.data, d_ptr.data_ptr(), M,
                                 BG_CODE.ctypes.data, tables.ptr, pv_ptr.ptr, n, ST())
    torch.cuda.synchronize()
    if status != 0:
        assert st == status
        assert tables.untouched() and pv_ptr.untouched()
        return lib.expecto_last_error().decode()
    assert st == 0, lib.expecto_last_error().decode()
    return tables.result(), pv_ptr.result()


# ---- expecto_pwm_pvalues -------------------------------------------------------------------------

@pytest.mark.parametrize("keys", [
    ((1, 0, False),), ((2, 0, False),), ((31, 0, False),), ((64, 0, False),),
    ((5, 0, True),), ((64, 1, True),),
    ((1, 1, False), (64, 0, False), (2, 1, False), (31, 0, False), (1, 2, True), (7, 0, False), (64, 1, True)),
    tuple((1 + k % 9, k, k % 5 == 0) for k in range(40)),
], ids=["w1", "w2", "w31", "w64", "flat5", "flat64", "mixed7", "many40"])
def test_pvalue_tables_are_the_sequential_scatter(lib, keys):
    mats = [motif(*k) for k in keys]
    pssm, col_ptr = pack(mats)
    tables, pv_ptr = pvalues_device(lib, pssm, col_ptr)
    want_ptr = np.concatenate([[0], np.cumsum([100 * m.shape[0] + 1 for m in mats])]).astype(np.int64)
    assert_bits(pv_ptr, want_ptr, "pv_ptr")
    assert want_ptr[-1] == tables.size            # back to back: a write past a table lands in its neighbour or the guard
    for i, k in enumerate(keys):
        assert_bits(tables[want_ptr[i]:want_ptr[i + 1]], ref_table(*k), f"table {i} of {k}")
        assert tables[want_ptr[i]] == 1.0 and (np.diff(tables[want_ptr[i]:want_ptr[i + 1]]) <= 0).all()


def test_pvalue_refusals(lib):
    ok = motif(3)
    for mats, edit, text in [
        ([ok, np.zeros((0, 4), np.int64), ok], None, "width 0"),
        ([ok, motif(64), ok], "widen", "width 65"),
        ([ok, ok], "entry", "outside 0..100"),
        ([ok, ok], "negative", "outside 0..100"),
        ([ok, ok, ok], "decrease", "decreasing"),
    ]:
        pssm, col_ptr = pack(mats)
        if edit == "widen":
            pssm, col_ptr = pack([ok, np.concatenate([motif(64), ok[:1]]), ok])
        elif edit == "entry":
            pssm[4, 2] = 101
        elif edit == "negative":
            pssm[0, 0] = -1
        elif edit == "decrease":
            col_ptr[2] = 2
        assert text in pvalues_device(lib, pssm, col_ptr, status=-1), (edit, lib.expecto_last_error())
    assert lib.expecto_pwm_pvalues(None, None, None, 2, None, None, None, 0, ST()) == -1
    assert "null" in lib.expecto_last_error().decode()
    assert lib.expecto_pwm_pvalues(None, None, None, 0, None, None, None, 0, ST()) == 0


# ---- expecto_pwm_scan ----------------------------------------------------------------------------

class Codes:
    """uint8 [S, L] on the device with row stride ld: codes 0..3 (never read) in the padding of a row,
    margins of code 4 before the first and after the last row."""

    def __init__(self, codes, ld, margin=512, seed=0):
        S, L = codes.shape
        ld = max(ld, L)                          # a stride below L is only ever refused
        host = np.full(2 * margin + S * ld, 4, np.uint8)
        body = host[margin:margin + S * ld].reshape(S, ld)
        body[:] = np.random.RandomState(seed).randint(0, 4, (S, ld))
        body[:, :L] = codes
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + margin


def fake_tables(mats, seed=0):
    """Any doubles serve the scan as tables: distinct ones show which entry was looked up."""
    rng = np.random.RandomState(seed)
    return [rng.rand(100 * m.shape[0] + 1) for m in mats]


def scan_device(lib, codes, overlap, mats, tables, ld=None, status=0, L=None):
    S, Lc = codes.shape
    L = Lc if L is None else L
    ld = Lc + 3 if ld is None else ld
    M = len(mats)
    pssm, col_ptr = pack(mats)
    flat = np.concatenate(tables) if tables else np.zeros(1)
    pv_ptr = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    src = Codes(codes, ld)
    keep = [dev(np.asarray(overlap, np.int32)) if S else None, dev(pssm) if pssm.size else None, dev(col_ptr), dev(flat),
            dev(pv_ptr)]
    d_ov, d_pssm, d_ptr, d_tab, d_pv = [None if t is None else t.data_ptr() for t in keep]
    n = max(1, S * M)
    outs = [Guarded((n,), np.int32), Guarded((n,), np.int32), Guarded((n,), np.uint8, offset=1), Guarded((n,), np.float64)]
    st = lib.expecto_pwm_scan(src.ptr, S, L, ld, d_ov, d_pssm, col_ptr.ctypes.data, d_ptr, M, d_tab, d_pv, flat.size,
                              *[o.ptr for o in outs], ST())
    torch.cuda.synchronize()
    if status != 0:
        assert st == status
        assert all(o.untouched() for o in outs)
        return lib.expecto_last_error().decode()
    assert st == 0, lib.expecto_last_error().decode()
    if S * M == 0:
        assert all(o.untouched() for o in outs)
        return None
    return tuple(o.result().reshape(S, M) for o in outs)


def assert_scan(lib, codes, overlap, mats, what, seed=0, **kw):
    tables = fake_tables(mats, seed)
    got = scan_device(lib, codes, overlap, mats, tables, **kw)
    L = kw.get("L") or codes.shape[1]
    want = fimo_ref.scan(codes, L, np.asarray(overlap), mats, tables)
    for g, w, name in zip(got, want, ("score", "start", "strand", "pvalue")):
        assert_bits(g, w, f"{what}: {name}")
    return want


def random_codes(S, L, seed=0, bad=0.0):
    rng = np.random.RandomState(seed)
    codes = rng.randint(0, 4, (S, L)).astype(np.uint8)
    if bad:
        codes[rng.rand(S, L) < bad] = 4
    return codes


def test_scan_flank_of_61_with_the_widths_at_its_edges(lib):
    """c = 30 in L = 61: widths 1 and 31 have all w windows, 32 loses one at each edge, 61 has the single
    window, 62 none."""
    mats = [motif(w) for w in (1, 31, 32, 61, 62)]
    codes = random_codes(3, 61, seed=1)
    score, start, strand, pvalue = assert_scan(lib, codes, [30, 30, 30], mats, "L=61")
    assert (score[:, 4] == -1).all() and (start[:, 4] == -1).all() and np.isnan(pvalue[:, 4]).all()
    assert (start[:, 3] == 0).all() and (start[:, 0] == 30).all() and (score[:, :4] >= 0).all()


@pytest.mark.parametrize("L,overlap", [(61, [-1, -1, -1, -1]), (61, [0, 60, 0, 60]), (61, [-1, 0, 30, 60]), (1, [0, -1, 0, 0]),
                                       (256, [255, 0, 128, -1]), (200, [63, 64, 127, 128])],
                         ids=["any", "ends", "mixed", "L1", "L256", "mask_words"])
def test_scan_geometries(lib, L, overlap):
    mats = [motif(w) for w in (1, 2, 5, 17, 33, 64)]
    codes = random_codes(4, L, seed=L, bad=0.02 if L > 100 else 0.0)
    want = assert_scan(lib, codes, overlap, mats, f"L={L} c={overlap}", ld=L + 7)
    if L == 1:
        assert (want[0][:, 0] >= 0).all() and (want[0][:, 1:] == -1).all()


def test_scan_refusals_and_empty_calls(lib):
    mats = [motif(3), motif(4)]
    tables = fake_tables(mats)
    codes = random_codes(2, 256)
    wide = np.concatenate([codes, codes[:, :1]], axis=1)
    assert "[1, 256]" in scan_device(lib, wide, [0, 0], mats, tables, status=-1)
    assert "ld < L" in scan_device(lib, codes, [0, 0], mats, tables, ld=255, status=-1)
    assert "width" in scan_device(lib, codes, [0, 0], [motif(3), np.zeros((0, 4), np.int64)], tables, status=-1)
    assert scan_device(lib, codes[:0], [], mats, tables) is None
    assert scan_device(lib, codes, [0, 0], [], []) is None
    assert lib.expecto_pwm_scan(None, 1, 5, 5, None, None, None, None, 1, None, None, 0, None, None, None, None, ST()) == -1
    assert "null" in lib.expecto_last_error().decode()


def test_scan_row_padding_is_never_read(lib):
    """ld > L: the padding holds bases, and L = 10 of a 20-column array leaves ten more of them unread."""
    mats = [motif(w) for w in (1, 4, 10, 11)]
    codes = random_codes(5, 20, seed=3)
    assert_scan(lib, codes, [-1, 9, 0, 5, -1], mats, "L=10 of 20", ld=33, L=10)


def test_scan_bad_bases(lib):
    L, c = 21, 10
    mats = [motif(w) for w in (1, 2, 6, 11)]
    codes = random_codes(6, L, seed=4)
    codes[0, c] = 4                          # at c: nothing is admissible
    codes[1, c - 1] = 4                      # next to c: the windows that end or start at c remain
    codes[2, c + 1] = 4
    codes[3, [c - 1, c + 1]] = 4             # only the width-1 window remains
    codes[4, 0] = 255                        # far from c: only the longest motif's first window goes
    want = assert_scan(lib, codes, [c] * 6, mats, "bad bases")
    assert (want[0][0] == -1).all() and np.isnan(want[3][0]).all()
    assert want[0][3, 0] >= 0 and (want[0][3, 1:] == -1).all()
    assert (want[1][1, 1:] >= c).all() and (want[1][2, 1:] + np.array([2, 6, 11]) - 1 <= c).all()
    # a bad base in every window of the best strand's best match: the result moves to another window
    m = motif(6)
    clean = random_codes(1, L, seed=5)
    best = fimo_ref.scan_one(m, clean[0].tolist(), L, -1)
    hit = clean.copy()
    hit[0, best[1] + 2] = 4
    moved = assert_scan(lib, np.concatenate([clean, hit]), [-1, -1], [m], "best window lost")
    assert moved[1][0, 0] == best[1] and not moved[1][1, 0] <= best[1] + 2 <= moved[1][1, 0] + 5


@pytest.mark.parametrize("S", [SEQ_TILE - 1, SEQ_TILE, SEQ_TILE + 1])
@pytest.mark.parametrize("M", [MOTIF_TILE - 1, MOTIF_TILE, MOTIF_TILE + 1])
def test_scan_at_the_tile_edges(lib, S, M):
    """Mixed widths inside one motif tile, the last tile short in either direction; per-sequence overlaps."""
    widths = [1, 8, 3, 12, 2, 7, 12, 1, 5, 9, 4, 11, 6, 10, 2, 3, 8]
    mats = [motif(w, seed=k) for k, w in enumerate(widths[:M])]
    codes = random_codes(S, 12, seed=S * 31 + M, bad=0.03)
    overlap = np.random.RandomState(S + M).randint(-1, 12, S)
    assert_scan(lib, codes, overlap, mats, f"S={S} M={M}")


def test_scan_ties_across_positions_and_strands(lib):
    half = np.array([[90, 5, 3, 2], [4, 80, 10, 6]])
    palindrome = np.concatenate([half, half[::-1, ::-1]])
    flat = np.full((3, 4), 50, np.int64)
    two = np.array([[100, 0, 0, 100], [0, 100, 100, 0]])          # A or T, then G or C: many equal windows
    codes = np.array([fimo_ref.codes_of(s) for s in ("AGCTAGCTAGCT", "ACACACACACAC", "TTTTGGGGAAAA", "AGCTNAGCTAGC")], np.uint8)
    want = assert_scan(lib, codes, [-1, -1, 5, -1], [palindrome, flat, two], "ties")
    assert want[1][0].tolist() == [0, 0, 0] and want[2][0].tolist() == [0, 0, 0]      # smallest start, '+'
    assert want[1][3, 0] == 0 and want[1][3, 1] == 0
    assert want[1][2, 1] == 3                                                            # the first window over c = 5


# ---- Python and the command lines ----------------------------------------------------------------

def test_python_api_tables_and_scan(q, lib):
    rng = np.random.RandomState(11)
    freqs = [rng.dirichlet(np.full(4, 0.4), w) for w in (4, 9, 1, 30)]
    meme = q.Meme(None, [f"M{i}" for i in range(4)], ["a", "b", "", "d"], freqs, [20.0, 7.0, 20.0, 100.0])
    bg = q.background("nrdb")
    motifs = q.Motifs.from_meme(meme, bg)
    tables = q.pvalue_tables(motifs, bg)
    mats = [motifs.pssm[a:b].astype(np.int64) for a, b in zip(motifs.col_ptr[:-1], motifs.col_ptr[1:])]
    want_tables = [fimo_ref.pvalue_table(m[:, fimo_ref.TO_CODE_ORDER], bg, gather=False) for m in mats]
    assert_bits(tables.tables.cpu().numpy(), np.concatenate(want_tables), "tables")
    codes = random_codes(70, 61, seed=12, bad=0.01)
    got = q.scan(codes, 30, motifs, tables)
    want = fimo_ref.scan(codes, 61, np.full(70, 30), mats, want_tables)
    for g, w, name in zip(got, want, ("score", "start", "strand", "pvalue")):
        assert_bits(g.cpu().numpy(), w, name)
    thr = float(np.nanmedian(want[3]))
    ptr, idx = q.matches_csr(got[3], thr)
    keep = want[3] < thr
    assert_bits(ptr, np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), "seq_ptr")
    assert_bits(idx, np.nonzero(keep)[1].astype(np.int32), "motif_idx")
    ptr2, idx2 = q.matches_csr(got[3], thr, motif_map=[5, -1, 0, 2])
    keep2 = keep & (np.array([5, -1, 0, 2]) >= 0)[None, :]
    assert_bits(ptr2, np.concatenate([[0], np.cumsum(keep2.sum(1))]).astype(np.int64), "mapped seq_ptr")
    assert_bits(idx2, np.array([5, -1, 0, 2], np.int32)[np.nonzero(keep2)[1]], "mapped motif_idx")
    with pytest.raises(ValueError, match="symmetric"):
        q.pvalue_tables(motifs, np.array(fimo_ref.NRDB))
    with pytest.raises(ValueError, match="1..256"):
        q.scan(random_codes(2, 257), 0, motifs, tables)


def write_inputs(root, seed=0):
    """A two-contig FASTA with lower-case stretches and an N run, 12 variants, 5 motifs."""
    rng = np.random.RandomState(seed)
    contigs = {}
    for name, n in (("chr1", 400), ("chr2", 260)):
        s = np.array(list("ACGT"))[rng.randint(0, 4, n)]
        contigs[name] = "".join(s)
    c1 = contigs["chr1"]
    contigs["chr1"] = c1[:60] + c1[60:130].lower() + c1[130:200] + "N" * 12 + c1[212:300] + c1[300:].lower()
    with open(root / "g.fa", "w") as f:
        for name, s in contigs.items():
            f.write(f">{name} test\n")
            f.writelines(s[i:i + 50] + "\n" for i in range(0, len(s), 50))
    places = [("chr1", 31), ("chr1", 45), ("chr1", 70), ("chr1", 128), ("chr1", 190), ("chr1", 225), ("chr1", 230),
              ("chr1", 320), ("chr1", 370), ("chr2", 31), ("chr2", 100), ("chr2", 230)]
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    with open(root / "v.vcf", "w") as f:
        f.write("##fileformat=VCFv4.0\n#CHROM\tPOS\tID\tREF\tALT\n")
        for k, (chrom, pos) in enumerate(places):
            base = contigs[chrom][pos - 1].upper()
            ref, alt = (base, other[base]) if k % 3 else (other[base], base)      # every third: only ALT is the genome's
            f.write(f"{chrom}\t{pos}\trs{k}\t{ref}\t{alt}\n")
    with open(root / "m.meme", "w") as f:
        f.write("MEME version 4\n\nALPHABET= ACGT\n\nBackground letter frequencies\nA 0.3 C 0.2 G 0.2 T 0.3\n\n")
        for k, w in enumerate((6, 10, 4, 15, 8)):
            f.write(f"MOTIF ID{k} ALT{k}\nletter-probability matrix: alength= 4 w= {w} nsites= {10 + k}\n")
            for row in rng.dirichlet(np.full(4, 0.3), w):
                row = np.round(row, 6)
                row[np.argmax(row)] += 1.0 - row.sum()
                f.write(" ".join(f"{x:.6f}" for x in row) + "\n")
            f.write("\n")
    return contigs, places


def query_args(q, root, out, *extra):
    return q.build_parser().parse_args(["--vcf_file", str(root / "v.vcf"), "--motif_file", str(root / "m.meme"),
                                        "--hg19_fasta", str(root / "g.fa"), "-o", str(out), *extra])


def test_query_cli_writes_the_restatements_rows(q, tmp_path):
    contigs, places = write_inputs(tmp_path)
    df = q.run(query_args(q, tmp_path, tmp_path / "whole", "--seq-batch", "5"))
    names = [f"rs{k}" for k in range(12)]
    seqs = [contigs[c][p - 31:p + 30].upper() for c, p in places]
    assert any("N" in s for s in seqs) and all(len(s) == 61 for s in seqs)
    _, ref_motifs = fimo_ref.parse_meme(str(tmp_path / "m.meme"))
    want = fimo_ref.filtered_rows(names, seqs, ref_motifs, BG, 30)
    assert len(want) > 50
    lines = open(tmp_path / "whole" / "fimo_filtered.tsv").read().splitlines()
    assert lines[0] == "\t" + "\t".join(fimo_ref.FIMO_COLUMNS)
    assert lines[1:] == [f"{i}\t{fimo_ref.text_row(r)}" for i, r in enumerate(want)]
    assert [tuple(r) for r in df.itertuples(index=False)] == want
    text = open(tmp_path / "whole" / "fimo_out.txt").read().splitlines()
    assert text[0][0] == "#" and text[1:] == [fimo_ref.text_row(r) for r in want]
    # chunks of five variants concatenate to the whole
    parts = [q.run(query_args(q, tmp_path, tmp_path / f"c{i}", "--chunk_size", "5", "--chunk_i", str(i))) for i in range(3)]
    assert [len(p) for p in parts] != [0, 0, 0]
    joined = pd.concat(parts, ignore_index=True).sort_values(by="p-value", kind="stable").reset_index(drop=True)
    assert [tuple(r) for r in joined.itertuples(index=False)] == want
    # a threshold: the rows at or below it, and in fimo_out.txt one more row for every motif left without
    cut = float(sorted(r[7] for r in want)[7])
    low = q.run(query_args(q, tmp_path, tmp_path / "low", "--thresh", repr(cut), "--bgfile", "nrdb"))
    assert [tuple(r) for r in low.itertuples(index=False)] == [r for r in want if r[7] <= cut]
    back = pd.read_table(tmp_path / "low" / "fimo_out.txt", sep='\t', names=fimo_ref.FIMO_COLUMNS, comment='#')
    assert set(back["motif_alt_id"]) == {f"ALT{k}" for k in range(5)}
    absent = [k for k in range(5) if f"ID{k}" not in set(low["motif_id"])]
    assert len(back) == len(low) + len(absent)
    for k in absent:
        best = min((r for r in want if r[0] == f"ID{k}"), key=lambda r: r[7])
        assert fimo_ref.text_row(best) in open(tmp_path / "low" / "fimo_out.txt").read().splitlines()


def test_query_cli_refuses_bad_variants(q, tmp_path):
    contigs, _ = write_inputs(tmp_path)
    base = contigs["chr2"][99]
    wrong = [b for b in "ACGT" if b != base]
    (tmp_path / "v.vcf").write_text(f"chr2\t100\trsX\t{wrong[0]}\t{wrong[1]}\n")
    with pytest.raises(ValueError, match="rsX.*does not match"):
        q.run(query_args(q, tmp_path, tmp_path / "o"))
    for pos in (30, 231):
        (tmp_path / "v.vcf").write_text(f"chr2\t{pos}\trsY\t{contigs['chr2'][pos - 1]}\tA\n")
        with pytest.raises(ValueError, match="rsY.*leaves the contig"):
            q.run(query_args(q, tmp_path, tmp_path / "o"))


def test_cluster_analysis_routes_agree(q, tmp_path):
    """--motif_file (scan and compaction on the device) against --fimo_out_file fed the text the query
    command line wrote: equal counts and p-values."""
    from expecto_amd import cluster_analysis_with_fimo as caf
    contigs, places = write_inputs(tmp_path, seed=1)
    rng = np.random.RandomState(3)
    C = 4
    with open(tmp_path / "cluster_contribs.tsv", "w") as f:
        f.write("\t".join(["index", "0", "1", "2", "3", "4", "gene", "SED", "SED_PROPORTION",
                           *[f"cluster_{c + 1}" for c in range(C)], "cluster_-1"]) + "\n")
        for k, (chrom, pos) in enumerate(places):
            vals = rng.standard_normal(C + 1)
            f.write("\t".join([str(k), chrom, str(pos), f"rs{k}", "N", "N", f"G{k % 3}", repr(float(rng.standard_normal())),
                               repr(float(rng.rand())), *[repr(float(x)) for x in vals]]) + "\n")
    (tmp_path / "rsat_clusters.tsv").write_text("cluster_1\tALT0,ALT3\ncluster_2\tALT1\ncluster_3\tALT2\ncluster_4\tALT4\n"
                                                "cluster_-1\tUNPLACED\n")
    thr = 0.03
    whole = q.run(query_args(q, tmp_path, tmp_path / "query"))
    # the test's own inputs: no p-value within the text's %.3g rounding of the threshold, and matches on both sides
    exact = whole["p-value"].to_numpy()
    assert all((p < thr) == (float("%.3g" % p) < thr) for p in exact)
    assert 5 < int((exact < thr).sum()) < len(exact) - 5
    common = ["--cluster_contribs_file", str(tmp_path / "cluster_contribs.tsv"), "--rsat_clusters_file",
              str(tmp_path / "rsat_clusters.tsv"), "--pval_match_threshold", repr(thr), "--n_neg_clusters", "2"]
    a, _ = caf.run(caf.build_parser().parse_args(common + ["--fimo_out_file", str(tmp_path / "query" / "fimo_out.txt"), "-o",
                                                           str(tmp_path / "a")]), out=io.StringIO())
    b, _ = caf.run(caf.build_parser().parse_args(common + ["--motif_file", str(tmp_path / "m.meme"), "--vcf_file",
                                                           str(tmp_path / "v.vcf"), "--hg19_fasta", str(tmp_path / "g.fa"),
                                                           "--seq-batch", "7", "-o", str(tmp_path / "b")]), out=io.StringIO())
    assert a.pos_matches.shape == (7, 3) and a.pos_matches.sum() > 0 and a.neg_matches.sum() > 0
    for x, y, name in zip(a, b, a._fields):
        assert_bits(x, y, name)
    assert open(tmp_path / "a" / "hypergeom.tsv").read() == open(tmp_path / "b" / "hypergeom.tsv").read()
