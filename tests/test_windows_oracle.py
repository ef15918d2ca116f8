"""CPU: the window oracle (oracle/windows_np.py, the reference of tests/test_gpu_hbm_kernels.py)
against what the project already trusts on a toy genome: the host twin ``pipeline.fetch_window``
+ ``seq_codes`` (chromatin.py:164,202-209), ``oracle.encode_np.tss_window`` and the
``CodeGenome`` slices of tests/test_host.py, for SNV, TSS, segment and indel cases inside a
contig; and the out-of-range code at both ends of the genome, which no contig-interior case
reads."""
import numpy as np
import pytest

from oracle import windows_np as wn


@pytest.fixture(scope="module")
def toy():
    from expecto_amd import synthetic
    from expecto_amd.genome import CodeGenome, Fasta
    g = synthetic.genome_bytes(n_contigs=2, contig_len=9000, seed=11)
    fa = Fasta.from_dict(g)
    return g, fa, CodeGenome(fa)


def _other_base(b: str, k: int = 1) -> str:
    return "AGCT"[("AGCT".index(b.upper()) + k) % 4] if b.upper() in "AGCT" else "A"


def test_read_pads_both_ends_with_the_outside_code():
    g = np.arange(10, dtype=np.uint8) % 4
    assert wn.read(g, -3, 5).tolist() == [4, 4, 4, 0, 1]
    assert wn.read(g, 8, 4).tolist() == [0, 1, 4, 4]
    assert wn.read(g, -2, 14).tolist() == [4, 4] + g.tolist() + [4, 4]
    assert wn.read(g, -7, 4).tolist() == [4] * 4 and wn.read(g, 10, 3).tolist() == [4] * 3
    assert wn.read(g, 2, 3).tolist() == [2, 3, 0]


def test_variant_windows_equal_fetch_window(toy):
    from expecto_amd.encode import seq_codes
    from expecto_amd.pipeline import _allele_code, fetch_window
    g, fa, cg = toy
    shifts = [0, -200, 200, -3, 7, 800, -800]
    pos = [2100, 4500, 4503, 6900]
    ref = [_other_base(chr(g["chr2"][p - 1])) for p in pos]           # a ref that mismatches the genome
    alt = [_other_base(chr(g["chr2"][p - 1]), 2) for p in pos]
    got = wn.variant_windows(cg.codes, [cg.offset("chr2", p) for p in pos], [_allele_code(c) for c in ref],
                             [_allele_code(c) for c in alt], shifts)
    assert got.shape == (2, len(shifts), len(pos), 2000)
    for a, alleles in enumerate((ref, alt)):
        for j, sh in enumerate(shifts):
            for v, p in enumerate(pos):
                want = seq_codes(fetch_window(fa, "chr2", p, ref[v], alleles[v], sh))
                assert np.array_equal(got[a, j, v], want), (a, sh, p)
                assert got[a, j, v, 999 - sh] == _allele_code(alleles[v])


def test_variant_allele_outside_the_window_changes_nothing():
    g = (np.arange(6000) % 4).astype(np.uint8)
    w = wn.variant_windows(g, [3000], [4], [4], [1000, 1001, -1000, -1001])
    assert w[0, 0, 0].tolist() == g[3001:5001].tolist() and w[0, 1, 0].tolist() == g[3002:5002].tolist()
    assert w[0, 2, 0, 1999] == 4 and w[0, 2, 0, :1999].tolist() == g[1001:3000].tolist()
    assert w[0, 3, 0].tolist() == g[1000:3000].tolist()


def test_tss_windows_equal_reference_tiling(toy):
    from expecto_amd.encode import seq_codes
    from oracle.encode_np import tss_window
    g, fa, cg = toy
    tss, strand, shifts = [3000, 5200, 5200], [1, -1, 1], [-400, 0, 3, 200, -1800, 1800]
    got = wn.tss_windows(cg.codes, [cg.offset("chr1", t) for t in tss], strand, shifts)
    for k, (t, s) in enumerate(zip(tss, strand)):
        for j, sh in enumerate(shifts):
            assert np.array_equal(got[k, j], seq_codes(tss_window(fa, "chr1", t, s, sh))), (t, s, sh)


def test_gather_segments_hold_the_shifted_snv_windows(toy):
    """A spliced segment holds every shift's SNV window (the layout pipeline.prepare builds)."""
    from expecto_amd.encode import seq_codes
    from expecto_amd.pipeline import _allele_code, fetch_window
    g, fa, cg = toy
    shifts = [0, -200, -400, 200, 400]
    lo, L = min(shifts), 2000 + max(shifts) - min(shifts)
    pos = [3100, 5555]
    alt = [_other_base(chr(g["chr1"][p - 1])) for p in pos]
    start = [cg.offset("chr1", p) + lo - 999 for p in pos]
    plain = wn.gather_segments(cg.codes, start, L)
    seg = wn.gather_segments(cg.codes, start, L, [999 - lo] * 2, [_allele_code(c) for c in alt])
    for v, p in enumerate(pos):
        assert np.array_equal(plain[v], cg.codes[start[v]:start[v] + L])
        for sh in shifts:
            want = seq_codes(fetch_window(fa, "chr1", p, "N", alt[v], sh))
            assert np.array_equal(seg[v, sh - lo:sh - lo + 2000], want), (p, sh)
    same = wn.gather_segments(cg.codes, start, L, [-1, L], [0, 0])       # splices outside: nothing changes
    assert np.array_equal(same, plain)


@pytest.mark.parametrize("lref,lalt", [(1, 2), (1, 100), (50, 1), (3, 3), (101, 1), (2, 5), (7, 1)])
def test_indel_windows_equal_fetch_window(toy, lref, lalt):
    from expecto_amd.encode import seq_codes
    from expecto_amd.pipeline import _LUT, fetch_window
    g, fa, cg = toy
    rng = np.random.default_rng(100 * lref + lalt)
    items, want = [], []
    for pos in (2300, 4444, 6600):
        ref = g["chr2"][pos - 1:pos - 1 + lref].decode()
        alt = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, lalt))
        for sh in (0, -600, 200, 1000, -940):
            for allele in (ref, alt):
                ls = 2100 - lref + len(allele)
                items.append((cg.offsets["chr2"] + pos + sh - 1050, 1049 - sh, lref, len(allele), (ls - 2000) // 2,
                              _LUT[np.frombuffer(allele.encode(), np.uint8)]))
                want.append(seq_codes(fetch_window(fa, "chr2", pos, ref, allele, sh)))
    cols = list(zip(*items))
    got = wn.indel_windows(cg.codes, *cols[:5], cols[5])
    for k, w in enumerate(want):
        assert w.size == 2000 and np.array_equal(got[k], w), items[k][:5]
