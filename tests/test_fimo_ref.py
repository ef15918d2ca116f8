"""CPU: the numpy restatement of the motif scan (tests/fimo_ref.py) against brute-force enumeration, and the
host side of expecto_amd.query_fimo_for_predictions (parser, background, scaled matrix, table formats)
against the restatement.  No ``fimo`` binary exists to compare with: the model is the documented one."""
import functools

import numpy as np
import pandas as pd
import pytest

import fimo_ref
from guarded import assert_bits


@pytest.fixture(scope="module")
def q():
    from expecto_amd import query_fimo_for_predictions
    return query_fimo_for_predictions


BG = fimo_ref.symmetric(fimo_ref.NRDB)


def random_freqs(rng, w, sharp=1.0):
    f = rng.dirichlet(np.full(4, sharp), w)
    return f / f.sum(axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def random_pssm(w, seed=0, equal=False):
    rng = np.random.RandomState(100 * w + seed)
    s, _, _ = fimo_ref.build_pssm(random_freqs(rng, w, 0.5), 20, BG)
    if equal:                       # equal scaled entries inside a column: the gather's tie rule decides the order
        s[::2, 1] = s[::2, 0]
        s[1::3, 3] = s[1::3, 2]
        s[-1, :] = s[-1, 0]
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_pvalue_table_equals_enumeration(w):
    s = random_pssm(w)
    assert s.min() >= 0 and s.max() <= 100
    pv = fimo_ref.pvalue_table(s, BG, gather=False)
    exact = fimo_ref.pvalue_by_enumeration(s, BG)
    assert pv.shape == (100 * w + 1,)
    live = exact > 0
    assert (np.abs(pv[live] - np.minimum(exact[live], 1.0)) <= 1e-12 * exact[live]).all()
    assert (pv[~live] == 0).all()
    assert (np.diff(pv) <= 0).all()


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_pvalue_table_starts_at_one(w):
    """``pv[0] == 1``: every score is >= 0.  The chain of rounded adds with the clip alone does not give
    this, since the clip only removes an excess: with these motifs it ends at 0.9999999999999993 for w = 4 and
    0.9999999999999996 for w = 6 (exactly 1.0 for the other widths).  So the model stores ``pv[0] = 1.0`` after
    the clip, on the host and on the device; the chain's own value lies within 1e-12 of it."""
    s = random_pssm(w)
    for gather in (False, True):
        pv = fimo_ref.pvalue_table(s, BG, gather=gather)
        assert pv[0] == 1.0 and pv[1] <= 1.0
    pdf = fimo_ref.pdf_scatter(s, BG)
    chain = float(np.cumsum(pdf[::-1])[-1])              # the same adds in the same order
    print(f"w={w}: the chain ends at {chain!r}")
    assert abs(chain - 1.0) <= 1e-12


@pytest.mark.parametrize("w", range(1, 14))
@pytest.mark.parametrize("equal", [False, True])
def test_gather_order_equals_the_sequential_scatter(w, equal):
    s = random_pssm(w, seed=1, equal=equal)
    if equal and w > 1:
        assert any(len(set(row.tolist())) < 4 for row in s)
    assert_bits(fimo_ref.pdf_gather(s, BG), fimo_ref.pdf_scatter(s, BG), f"pdf w={w}")
    assert_bits(fimo_ref.pvalue_table(s, BG, gather=True), fimo_ref.pvalue_table(s, BG, gather=False), f"pv w={w}")


def test_uniform_motif_on_a_uniform_background(q):
    uniform = np.full(4, 0.25)
    for build in (fimo_ref.build_pssm, q.build_pssm):
        s, scale, offset = build(np.full((3, 4), 0.25), 20, uniform)
        assert (np.asarray(s) == 100).all() and scale == 100.0 and abs(offset + 1.0) < 1e-12
    pv = fimo_ref.pvalue_table(np.asarray(s), uniform)
    assert (pv == 1.0).all() and pv.shape == (301,)


def test_build_pssm_is_the_restatement(q):
    rng = np.random.RandomState(5)
    for w in (1, 7, 30):
        f = random_freqs(rng, w, 0.3)
        f[0] = [1.0, 0.0, 0.0, 0.0]                      # a zero frequency lives on the pseudocount
        for nsites, pseudo in ((20, 0.1), (3.5, 0.01), (1000, 1.0)):
            got, want = q.build_pssm(f, nsites, BG, pseudo), fimo_ref.build_pssm(f, nsites, BG, pseudo)
            assert_bits(np.asarray(got[0], np.int64), want[0], "scaled matrix")
            assert got[1] == want[1] and got[2] == want[2]
            assert want[0].min() == 0 and want[0].max() == 100
    with pytest.raises(ValueError, match="symmetric"):
        q.build_pssm(f, 20, np.array(fimo_ref.NRDB))
    with pytest.raises(ValueError, match="shape"):
        q.build_pssm(np.zeros((0, 4)), 20, BG)


def test_minus_strand_is_the_plus_strand_of_the_reverse_complement():
    rng = np.random.RandomState(7)
    s_code = random_pssm(9, seed=2)[:, fimo_ref.TO_CODE_ORDER]
    for _ in range(20):
        codes = rng.randint(0, 4, 15).tolist()
        rc = [3 - c for c in codes[::-1]]
        for p in range(15 - 9 + 1):
            plus, minus = fimo_ref.strand_scores(s_code, codes, p)
            plus_rc, minus_rc = fimo_ref.strand_scores(s_code, rc, 15 - 9 - p)
            assert minus == plus_rc and plus == minus_rc
    # the letters agree with the codes: A <-> T, C <-> G
    assert fimo_ref.revcomp("AACGT") == "ACGTT"
    assert [3 - c for c in fimo_ref.codes_of("AACGT")[::-1]] == fimo_ref.codes_of("ACGTT")


def test_ties_take_the_smaller_start_and_the_plus_strand():
    # a palindromic motif (column i equals the complement of column w-1-i) on a palindromic sequence
    half = np.array([[90, 5, 3, 2], [4, 80, 10, 6]])                       # code order
    s_code = np.concatenate([half, half[::-1, ::-1]])
    seq = "AGCTAGCT"
    assert fimo_ref.revcomp(seq) == seq
    codes = fimo_ref.codes_of(seq)
    scores = [fimo_ref.strand_scores(s_code, codes, p) for p in range(5)]
    assert all(a == b for a, b in scores) and scores[0] == scores[4] == max(scores)
    assert fimo_ref.scan_one(s_code, codes, 8, -1) == (scores[0][0], 0, 0)
    assert fimo_ref.scan_one(s_code, codes, 8, 5) == (scores[4][0], 4, 0)   # only the windows over position 5
    assert fimo_ref.scan_one(s_code, codes, 3, -1) == (-1, -1, 0)           # the motif is longer than the sequence
    bad = list(codes)
    bad[2] = 4
    assert fimo_ref.scan_one(s_code, bad, 8, -1) == (scores[4][0], 4, 0)    # windows 0..2 hold the bad base
    assert fimo_ref.scan_one(s_code, bad, 8, 2) == (-1, -1, 0)              # and so does every window over it


# ---- parser --------------------------------------------------------------------------------------

MEME = """MEME version 4

ALPHABET= ACGT

strands: + -

Background letter frequencies (from uniform background):
A 0.30 C 0.20 G 0.22 T 0.28

MOTIF M1 alt_one
letter-probability matrix: alength= 4 w= 2 nsites= 35 E= 1e-3
0.7 0.1 0.1 0.1
0.25 0.25 0.25 0.25
URL http://example.invalid/M1

MOTIF M2
letter-probability matrix: alength= 4 w= 3
 0.1  0.2  0.3  0.4
 0.001 0.001 0.997 0.001
 1 0 0 0

MOTIF M3 alt_three
letter-probability matrix: alength= 4 w= 1 nsites= 0
0.4 0.3 0.2 0.1
"""


def test_parser_reads_the_minimal_format(q, tmp_path):
    path = tmp_path / "m.meme"
    path.write_text(MEME)
    meme = q.read_meme(str(path))
    assert meme.ids == ["M1", "M2", "M3"] and meme.alt_ids == ["alt_one", "", "alt_three"]
    assert meme.nsites == [35.0, 20.0, 20.0]
    assert [f.shape for f in meme.freqs] == [(2, 4), (3, 4), (1, 4)]
    assert meme.freqs[1][1].tolist() == [0.001, 0.001, 0.997, 0.001]
    assert meme.background.tolist() == [0.30, 0.20, 0.22, 0.28]
    ref_bg, ref_motifs = fimo_ref.parse_meme(str(path))
    assert ref_bg.tolist() == meme.background.tolist()
    for (mid, alt, f, n), i in zip(ref_motifs, range(3)):
        assert (mid, alt, n) == (meme.ids[i], meme.alt_ids[i], meme.nsites[i]) and (f == meme.freqs[i]).all()
    # backgrounds: symmetric, alphabet order
    assert_bits(q.background("motif-file", meme), fimo_ref.symmetric([0.30, 0.20, 0.22, 0.28]), "motif-file")
    assert_bits(q.background("nrdb"), BG, "nrdb")
    assert q.background("uniform").tolist() == [0.25] * 4
    bgfile = tmp_path / "bg.txt"
    bgfile.write_text("# order 0\nA 0.29\nC 0.21\nG 0.19\nT 0.31\nAA 0.1\n")
    assert_bits(q.background(str(bgfile)), fimo_ref.symmetric([0.29, 0.21, 0.19, 0.31]), "file")
    bg = q.background("nrdb")
    assert bg[0] == bg[3] and bg[1] == bg[2]
    # packed for the device: code order, widths, one scale and offset per motif
    motifs = q.Motifs.from_meme(meme, bg)
    assert motifs.col_ptr.tolist() == [0, 2, 5, 6] and motifs.pssm.dtype == np.int16 and len(motifs) == 3
    s, scale, offset = fimo_ref.build_pssm(meme.freqs[1], 20.0, bg)
    assert_bits(motifs.pssm[2:5].astype(np.int64), s[:, fimo_ref.TO_CODE_ORDER], "packed")
    assert motifs.scales[1] == scale and motifs.offsets[1] == offset


@pytest.mark.parametrize("old,new,message", [
    ("alength= 4 w= 2", "alength= 20 w= 2", "M1.*alength"),
    ("0.25 0.25 0.25 0.25\n", "", "M1.*rows"),
    ("0.7 0.1 0.1 0.1", "0.7 0.1 0.1 0.2", "M1.*sums"),
    (" 1 0 0 0\n", "", "M2.*rows"),
    ("letter-probability matrix: alength= 4 w= 1 nsites= 0\n0.4 0.3 0.2 0.1\n", "", "M3.*no letter-probability"),
])
def test_parser_refuses(q, tmp_path, old, new, message):
    assert old in MEME
    path = tmp_path / "bad.meme"
    path.write_text(MEME.replace(old, new))
    with pytest.raises(ValueError, match=message):
        q.read_meme(str(path))


def test_backgrounds_refused(q, tmp_path):
    path = tmp_path / "m.meme"
    path.write_text(MEME.replace("Background letter frequencies (from uniform background):\nA 0.30 C 0.20 G 0.22 T 0.28\n", ""))
    with pytest.raises(ValueError, match="motif-file"):
        q.background("motif-file", q.read_meme(str(path)))
    short = tmp_path / "bg.txt"
    short.write_text("A 0.5\nC 0.5\n")
    with pytest.raises(ValueError, match="A C G T"):
        q.background(str(short))
    wide = q.Meme(None, ["LONG"], [""], [np.full((65, 4), 0.25)], [20.0])
    with pytest.raises(ValueError, match="LONG.*65"):
        q.Motifs.from_meme(wide, BG)


# ---- tables --------------------------------------------------------------------------------------

def small_run(q, tmp_path):
    """Three sequences, the three motifs of MEME, the scan by the restatement."""
    path = tmp_path / "m.meme"
    path.write_text(MEME)
    meme = q.read_meme(str(path))
    bg = q.background("nrdb")
    motifs = q.Motifs.from_meme(meme, bg)
    names, seqs = ["rs1", "rs2", "rs3"], ["ACGTACG", "TTTTTTT", "GGNAGGC"]
    codes = np.array([fimo_ref.codes_of(s) for s in seqs], np.uint8)
    mats = [motifs.pssm[a:b].astype(np.int64) for a, b in zip(motifs.col_ptr[:-1], motifs.col_ptr[1:])]
    tables = [fimo_ref.pvalue_table(m[:, fimo_ref.TO_CODE_ORDER], bg) for m in mats]    # code order back to alphabet order
    res = fimo_ref.scan(codes, 7, np.full(3, 3), mats, tables)
    _, ref_motifs = fimo_ref.parse_meme(str(path))
    return names, seqs, motifs, res, fimo_ref.filtered_rows(names, seqs, ref_motifs, bg, 3)


def test_best_matches_columns_and_coordinates(q, tmp_path):
    names, seqs, motifs, res, want = small_run(q, tmp_path)
    df = q.best_matches(names, seqs, motifs, *res)
    assert list(df.columns) == fimo_ref.FIMO_COLUMNS
    got = [tuple(r) for r in df.itertuples(index=False)]
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert (df["p-value"].to_numpy()[:-1] <= df["p-value"].to_numpy()[1:]).all()
    assert set(df["strand"]) == {"+", "-"} and (df["q-value"] == "").all()
    for r in df.itertuples(index=False):
        seq = seqs[names.index(r[2])]
        window = seq[r[3] - 1:r[4]]                                      # 1-based, inclusive
        assert r[3] <= 4 <= r[4] and "N" not in window
        assert r[9] == (window if r[5] == "+" else fimo_ref.revcomp(window))
        m = motifs.ids.index(r[0])
        assert r[4] - r[3] + 1 == motifs.widths[m]
    # the third sequence has an N at position 3: of the windows over position 4, motif M2 (w = 3) keeps one
    assert (df[df["sequence_name"] == "rs3"]["start"] >= 4).all()
    # a threshold keeps the rows at or below it
    cut = float(np.median(df["p-value"]))
    assert len(q.best_matches(names, seqs, motifs, *res, thresh=cut)) == int((df["p-value"] <= cut).sum())


def test_files_round_trip_through_the_reference_reader(q, tmp_path):
    names, seqs, motifs, res, want = small_run(q, tmp_path)
    df = q.best_matches(names, seqs, motifs, *res)
    q.write_fimo_text(df, str(tmp_path / "fimo_out.txt"))
    q.write_filtered(df, str(tmp_path / "fimo_filtered.tsv"))
    text = open(tmp_path / "fimo_out.txt").read().splitlines()
    assert text[0].startswith("# motif_id\t") and text[1:] == [fimo_ref.text_row(r) for r in want]
    back = pd.read_table(tmp_path / "fimo_out.txt", sep='\t', names=fimo_ref.FIMO_COLUMNS, comment='#')
    assert len(back) == len(df)
    assert back["motif_id"].tolist() == df["motif_id"].tolist()
    assert back["motif_alt_id"].fillna("").tolist() == df["motif_alt_id"].tolist()
    assert back["start"].tolist() == df["start"].tolist() and back["stop"].tolist() == df["stop"].tolist()
    assert back["strand"].tolist() == df["strand"].tolist()
    assert back["matched_sequence"].tolist() == df["matched_sequence"].tolist()
    assert back["q-value"].isna().all()
    assert back["p-value"].tolist() == [float("%.3g" % p) for p in df["p-value"]]
    assert back["score"].tolist() == [float("%g" % s) for s in df["score"]]
    filt = pd.read_csv(tmp_path / "fimo_filtered.tsv", sep="\t", index_col=0)
    assert list(filt.columns) == fimo_ref.FIMO_COLUMNS and filt.index.tolist() == list(range(len(df)))
    assert filt["sequence_name"].tolist() == df["sequence_name"].tolist()


def test_cluster_analysis_wants_one_route():
    from expecto_amd import cluster_analysis_with_fimo as caf
    base = ["--cluster_contribs_file", "a", "--rsat_clusters_file", "b"]
    for extra in ([], ["--fimo_out_file", "f", "--motif_file", "m", "--vcf_file", "v"], ["--motif_file", "m"]):
        with pytest.raises(SystemExit) as e:
            caf.main(base + extra)
        assert e.value.code == 2
    args = caf.build_parser().parse_args(base + ["--fimo_out_file", "f"])
    assert caf.route_error(args) is None and args.motif_file is None
