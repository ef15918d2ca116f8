"""Edge tests of the HBM-bound kernels of reduce.hip, called through the C entry points.

Every output is carved out of a larger device buffer filled with a byte pattern (``Guarded``):
the intended region must equal the reference and every byte around it must keep the pattern,
so a store one slot outside the output fails the test.  Comparisons are bitwise through the
integer views of the floats (``assert_bits``: NaNs match as NaNs, -0.0 differs from 0.0); the
one exception is the device-``exp`` branch, which has a derived bound.

References: oracle/windows_np.py (window codes), numpy ``a - b`` (diff),
oracle.reduce_np (averages, TSS / variant reductions), oracle.gblinear_np (scoring).  The
TSS / shift reductions' oracle is numpy's sum over the shift axis of 2002-wide rows: it starts
from +0.0 and adds the products in order (``_tss_ref`` keeps that order for a 1-wide row, where
numpy would switch to its pairwise inner loop, which the reference programs never run).  The
variant reduction's oracle adds from the first term, as predict.py's functools.reduce: a sum
of -0.0 terms (negative effects under a masked weight) is -0.0 there and +0.0 in a TSS sum.
The inputs of both are signed, with exact zeros of both signs, so both conventions show."""
import numpy as np
import pytest
import torch

from guarded import Guarded, P, ST, assert_bits, dev, dev_offset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


def last_error(lib):
    return lib.expecto_last_error().decode()


# ---- window kernels ------------------------------------------------------------------------

GLEN = 5003                                  # not a multiple of 4; windows run off both ends
EDGE_OFFSETS = [0, 5, 998, 999, 1000, GLEN - 1001, GLEN - 1000, GLEN - 1]


@pytest.fixture(scope="module")
def genome():
    g = np.random.default_rng(50).integers(0, 5, GLEN).astype(np.uint8)
    return g, dev(g)


def _call_variant_windows(lib, gd, glen, off, rc, ac, shifts):
    n, S = len(off), len(shifts)
    out = Guarded((2, S, n, 2000), np.uint8)
    args = [dev(np.asarray(x, t)) for x, t in ((off, np.int64), (rc, np.uint8), (ac, np.uint8), (shifts, np.int32))]
    st = lib.expecto_variant_windows(P(gd), glen, P(args[0]), P(args[1]), P(args[2]), n, P(args[3]), S, out.ptr, ST())
    assert st == 0, last_error(lib)
    return out.result()


VARIANT_SHIFTS = [0, -3, 7, 999, -1000, 1001, -1001]   # variant at 999, 1002, 992, 0, 1999, outside, outside


@pytest.mark.parametrize("n", [1, 9])
def test_variant_windows_edges(lib, genome, n):
    """Windows off both ends of the genome (code 4), the variant at window index 0 and 1999, on
    and next to a 4-code word boundary (992, 999, 1002) and outside the window (shifts +-1001:
    no code replaced), ref / alt codes that differ from the genome's; n = 1: one call per offset."""
    from oracle.windows_np import variant_windows
    g, gd = genome
    offs = EDGE_OFFSETS + [2501]
    rc = [(int(g[o]) + 1) % 5 for o in offs]
    ac = [(int(g[o]) + 2) % 5 for o in offs]
    groups = [[k] for k in range(8)] if n == 1 else [list(range(9))]
    for grp in groups:
        o, r, a = ([x[k] for k in grp] for x in (offs, rc, ac))
        got = _call_variant_windows(lib, gd, GLEN, o, r, a, VARIANT_SHIFTS)
        assert_bits(got, variant_windows(g, o, r, a, VARIANT_SHIFTS), f"variant_windows offsets {o}")


def test_variant_windows_nothing_to_do(lib, genome):
    g, gd = genome
    out = Guarded((2, 7, 1, 2000), np.uint8)
    t = [dev(np.zeros(1, ty)) for ty in (np.int64, np.uint8, np.uint8)]
    sh = dev(np.asarray(VARIANT_SHIFTS, np.int32))
    assert lib.expecto_variant_windows(P(gd), GLEN, P(t[0]), P(t[1]), P(t[2]), 0, P(sh), 7, out.ptr, ST()) == 0
    assert out.untouched()


@pytest.mark.parametrize("shifts", [[-400, 0, 3, 200], [-400]])
def test_tss_windows_edges(lib, genome, shifts):
    from oracle.windows_np import tss_windows
    g, gd = genome
    off = EDGE_OFFSETS * 2
    strand = [1] * 8 + [-1] * 8
    out = Guarded((16, len(shifts), 2000), np.uint8)
    od, sd, hd = dev(np.asarray(off, np.int64)), dev(np.asarray(strand, np.int8)), dev(np.asarray(shifts, np.int32))
    st = lib.expecto_tss_windows(P(gd), GLEN, P(od), P(sd), 16, P(hd), len(shifts), out.ptr, ST())
    assert st == 0, last_error(lib)
    assert_bits(out.result(), tss_windows(g, off, strand, shifts), "tss_windows")


@pytest.mark.parametrize("seg_len", [4, 1028, 2000, 3600])
def test_gather_segments_edges(lib, genome, seg_len):
    """seg_len 1028: 257 word threads, the second 256-thread x-block has one live thread; 3600:
    four x-blocks.  Starts before, inside, across and past the genome; without a splice table
    (null splice_code), and with splices at 0, seg_len-1 and the out-of-segment -1 / seg_len."""
    from oracle.windows_np import gather_segments
    g, gd = genome
    start = [-2, -seg_len - 5, 17, 1001, GLEN - seg_len // 2, GLEN - 3, GLEN + 10, 2002]
    n = len(start)
    sd = dev(np.asarray(start, np.int64))
    plain = gather_segments(g, start, seg_len)
    out = Guarded((n, seg_len), np.uint8)
    assert lib.expecto_gather_segments(P(gd), GLEN, P(sd), n, seg_len, None, None, out.ptr, ST()) == 0, last_error(lib)
    assert_bits(out.result(), plain, "gather_segments, no splice")
    pos = [0, seg_len - 1, -1, seg_len, seg_len - 1, 0, seg_len // 2, seg_len]
    code = [(int(plain[i, p]) + 1) % 5 if 0 <= p < seg_len else 0 for i, p in enumerate(pos)]
    want = gather_segments(g, start, seg_len, pos, code)
    assert (want != plain).sum() == sum(0 <= p < seg_len for p in pos)
    assert np.array_equal(want[[2, 3, 7]], plain[[2, 3, 7]])            # -1 and seg_len change nothing
    out = Guarded((n, seg_len), np.uint8)
    pd, cd = dev(np.asarray(pos, np.int32)), dev(np.asarray(code, np.uint8))
    st = lib.expecto_gather_segments(P(gd), GLEN, P(sd), n, seg_len, P(pd), P(cd), out.ptr, ST())
    assert st == 0, last_error(lib)
    assert_bits(out.result(), want, "gather_segments, spliced")


def test_gather_segments_refuses_a_ragged_length(lib, genome):
    g, gd = genome
    out = Guarded((2, 1030), np.uint8)
    sd = dev(np.asarray([0, 100], np.int64))
    assert lib.expecto_gather_segments(P(gd), GLEN, P(sd), 2, 1030, None, None, out.ptr, ST()) == -1
    assert "seg_len % 4" in last_error(lib)
    assert out.untouched()


# (mutpos, lref, lalt): spliced length 2100 - lref + lalt, crop floor((length - 2000) / 2)
INDEL_CASES = [
    (1049, 50, 1),      # deletion
    (1049, 1, 100),     # insertion
    (1049, 3, 3),       # MNP
    (1049, 101, 1),     # spliced length exactly 2000, crop 0
    (0, 1, 5),          # mutpos 0, the allele ahead of the crop (52)
    (0, 1, 300),        # mutpos 0, the allele straddles the crop's start (199)
    (2090, 10, 3),      # mutpos + lref = 2100
    (60, 1, 100),       # allele 60..159 straddles the crop's start (99)
    (2050, 1, 100),     # allele 2050..2149 straddles the crop's end (99 + 2000)
    (1999, 101, 1),     # the deletion reaches the fetch window's last base, crop 0
]


def _indel_items(g, glen_local, cases, starts):
    items = []
    for k, (mp, lr, la) in enumerate(cases):
        s0 = starts[k % len(starts)]
        under = g[np.clip(s0 + mp + np.arange(la), 0, glen_local - 1)].astype(np.int64)
        allele = ((under + 1 + np.arange(la) % 2) % 5).astype(np.uint8)     # differs from the genome's codes
        items.append((s0, mp, lr, la, (2100 - lr + la - 2000) // 2, allele))
    return items


def _call_indel_windows(lib, gd, glen, items, start_base=0):
    n = len(items)
    table = np.concatenate([np.full(3, 4, np.uint8)] + [it[5] for it in items])       # offsets start at 3
    aoff = 3 + np.concatenate([[0], np.cumsum([it[5].size for it in items])[:-1]])
    cols = [dev(np.asarray([it[0] + start_base for it in items], np.int64))]
    cols += [dev(np.asarray([it[c] for it in items], np.int32)) for c in (1, 2, 3, 4)]
    cols += [dev(aoff.astype(np.int32)), dev(table)]
    out = Guarded((n, 2000), np.uint8)
    st = lib.expecto_indel_windows(P(gd), glen, *(P(c) for c in cols), n, out.ptr, ST())
    assert st == 0, last_error(lib)
    return out.result()


def test_indel_windows_edges(lib, genome):
    """What test_indel_windows_device_equal_host_splice (random positions and alleles, mutpos
    249..1849 through the pipeline) does not reach: a spliced length of exactly 2000, mutpos 0,
    mutpos + lref = 2100, alleles that straddle either end of the crop; and a deletion, an
    insertion and an MNP whose allele codes all differ from the genome's codes under them.
    The fetch windows start at the genome's first base, inside, and end at its last base."""
    from oracle.windows_np import indel_windows
    g, gd = genome
    items = _indel_items(g, GLEN, INDEL_CASES, [0, 1234, GLEN - 2100, 77])
    got = _call_indel_windows(lib, gd, GLEN, items)
    cols = list(zip(*items))
    assert_bits(got, indel_windows(g, *cols[:5], cols[5]), "indel_windows")


def test_window_kernels_past_2_31(lib):
    """A genome of 2^31 + 8192 codes (hg19 has 3.1 G bases): windows of all four kernels that
    straddle offset 2^31 and that end at, or run past, the last base.  The reference reads only
    the last 16 KiB of the genome, copied back; an index narrowed to 32 bits reads elsewhere."""
    from oracle import windows_np as wn
    free, _ = torch.cuda.mem_get_info()
    if free < 4 << 30:
        pytest.skip(f"needs 4 GiB of free device memory for the 2 GiB genome, {free >> 20} MiB free")
    B = 1 << 31
    L = B + 8192
    gd = torch.empty(L, dtype=torch.uint8, device="cuda")
    piece = 1 << 28
    for i in range(0, L, piece):
        m = min(piece, L - i)
        gd[i:i + m] = torch.randint(0, 5, (m,), dtype=torch.uint8, device="cuda")
    base = B - 8192                                       # the slice the windows read
    tail = gd[base:].cpu().numpy()
    assert tail.size == 16384 and len(np.unique(tail)) == 5
    try:
        offs = [B - 1000, B - 1, B, B + 5, L - 1000, L - 1]
        loc = [o - base for o in offs]
        rc = [(int(tail[o]) + 1) % 5 for o in loc]
        ac = [(int(tail[o]) + 2) % 5 for o in loc]
        shifts = [0, -3, 7, 999]
        got = _call_variant_windows(lib, gd, L, offs, rc, ac, shifts)
        assert_bits(got, wn.variant_windows(tail, loc, rc, ac, shifts), "variant_windows past 2^31")

        strand, tsh = [1, -1] * 3, [-400, 0, 3, 200]
        out = Guarded((6, 4, 2000), np.uint8)
        od, sd, hd = dev(np.asarray(offs, np.int64)), dev(np.asarray(strand, np.int8)), dev(np.asarray(tsh, np.int32))
        assert lib.expecto_tss_windows(P(gd), L, P(od), P(sd), 6, P(hd), 4, out.ptr, ST()) == 0, last_error(lib)
        assert_bits(out.result(), wn.tss_windows(tail, loc, strand, tsh), "tss_windows past 2^31")

        start = [B - 1800, B - 4, B, L - 3600, L - 100]
        sloc = [s - base for s in start]
        pos = [1800, 3, 0, 3599, 50]
        plain = wn.gather_segments(tail, sloc, 3600)
        code = [(int(plain[i, p]) + 1) % 5 for i, p in enumerate(pos)]
        out = Guarded((5, 3600), np.uint8)
        sd, pd, cd = dev(np.asarray(start, np.int64)), dev(np.asarray(pos, np.int32)), dev(np.asarray(code, np.uint8))
        st = lib.expecto_gather_segments(P(gd), L, P(sd), 5, 3600, P(pd), P(cd), out.ptr, ST())
        assert st == 0, last_error(lib)
        assert_bits(out.result(), wn.gather_segments(tail, sloc, 3600, pos, code), "gather_segments past 2^31")

        items = _indel_items(tail, tail.size, INDEL_CASES, [B - 1050 - base, B - 2099 - base, L - 2100 - base, 8192])
        got = _call_indel_windows(lib, gd, L, items, start_base=base)
        cols = list(zip(*items))
        assert_bits(got, wn.indel_windows(tail, *cols[:5], cols[5]), "indel_windows past 2^31")
    finally:
        del gd
        torch.cuda.empty_cache()


# ---- diff and fwd/rc average ---------------------------------------------------------------

F32_MAX = np.finfo(np.float32).max
DEN = np.float32(1e-45)                     # the smallest float32 denormal
# (a, b) pairs: signed zeros, infinities (inf - inf = NaN), NaN, the largest finite float32
# (overflow and exact cancellation), denormals whose difference (and sum) is denormal
SPECIAL_PAIRS = np.array([
    (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 0.0), (np.inf, np.inf), (np.inf, -np.inf), (-np.inf, np.inf),
    (np.nan, 1.0), (1.0, np.nan), (F32_MAX, -F32_MAX), (F32_MAX, F32_MAX), (-F32_MAX, F32_MAX), (F32_MAX, 1.0),
    (3 * DEN, DEN), (DEN, 3 * DEN), (1e-38, 0.9e-38), (-1e-39, 2e-39), (1.5, 1.5), (-2.5, -2.5), (1e-39, -1e-39),
], np.float32)


def _plant(a, b, at, roll=0):
    """Write the special pairs into the flat float32 arrays a / b from index `at` (clipped)."""
    sp = np.roll(SPECIAL_PAIRS, -roll, axis=0)
    m = min(len(sp), a.size - at)
    if at >= 0 and m > 0:
        a[at:at + m], b[at:at + m] = sp[:m, 0], sp[:m, 1]


@pytest.fixture(scope="module")
def normals():
    n = 8192 * 256 * 4 + 5
    rng = np.random.default_rng(51)
    return rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)


WRAP4 = 8192 * 256 * 4                      # floats one pass of the float4 grid covers
WRAP1 = 8192 * 256                          # floats one pass of the scalar grid covers


@pytest.mark.parametrize("misalign", ["none", "alt", "out"])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, WRAP1 + 3, WRAP4 + 5])
def test_diff_paths(lib, normals, count, misalign):
    """expecto_diff picks its kernels on the host: alt, ref and out all 16-byte aligned -> the
    float4 kernel on count // 4 groups (8192 x 256 threads at most: count = 8192*256*4 + 5
    wraps its grid-stride loop once) plus the scalar kernel on the count % 4 tail; any pointer
    off 16 bytes (`alt` or `out` moved by 4) -> the scalar kernel alone (count = 8192*256 + 3
    wraps its loop).  Reference: numpy a - b in float32; a denormal flushed to zero fails."""
    for roll in ((0, 4, 9, 13, 16) if count < 20 else (count % 7,)):     # short inputs: several slices of the pairs
        a, b = (x[:count].copy() for x in normals)
        _plant(a, b, 0, roll=roll)
        _plant(a, b, count - len(SPECIAL_PAIRS), roll=3)
        for wrap in (WRAP1, WRAP4):
            if wrap < count:
                _plant(a, b, wrap - 8, roll=7)
        with np.errstate(invalid="ignore", over="ignore"):
            want = a - b
        ad = dev_offset(a, 4 if misalign == "alt" else 0)
        bd = dev_offset(b, 0)
        out = Guarded((count,), np.float32, offset=4 if misalign == "out" else 0)
        assert (out.ptr % 16 == 0) == (misalign != "out") and (ad.data_ptr() % 16 == 0) == (misalign != "alt")
        assert lib.expecto_diff(P(ad), P(bd), count, out.ptr, ST()) == 0, last_error(lib)
        got = out.result()
        assert_bits(got, want, f"diff count {count} roll {roll}")
        den = (want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)
        assert den.any() or roll in (0, 4, 9)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 7), (1, 2002), (1100, 2002)])
def test_fwd_rc_average_matches_oracle(lib, normals, rows, cols):
    """(1100, 2002) exceeds the 8192 x 256 threads of one pass of the grid-stride loop."""
    from oracle.reduce_np import fwd_rc_average
    total = rows * cols
    a, b = (x[:total].copy() for x in normals)
    _plant(a, b, 0, roll=rows)
    _plant(a, b, total - len(SPECIAL_PAIRS), roll=5)
    if total > WRAP1:
        _plant(a, b, WRAP1 - 8, roll=7)
    x = np.concatenate([a, b]).reshape(2 * rows, cols)
    with np.errstate(invalid="ignore", over="ignore"):
        want = fwd_rc_average(x)
    out = Guarded((rows, cols), np.float32)
    xd = dev(x)
    assert lib.expecto_fwd_rc_average(P(xd), rows, cols, out.ptr, ST()) == 0, last_error(lib)
    assert_bits(out.result(), want, f"fwd_rc_average {rows}x{cols}")


# ---- shift / TSS reductions ----------------------------------------------------------------

def _signed(rng, shape):
    """float32 normals of both signs with a few exact zeros of both signs."""
    x = rng.standard_normal(shape, dtype=np.float32)
    flat = x.reshape(-1)
    idx = rng.integers(0, flat.size, max(1, flat.size // 16))
    flat[idx] = np.where(rng.random(idx.size) < 0.5, np.float32(0.0), np.float32(-0.0))
    return x


def _masked_weights(rng, S):
    """[10, S] float64 like the decay weights: positive, and each shift counts upstream (rows
    0..4), downstream (rows 5..9) or on both sides; the other side's weights are exact zeros."""
    w = np.exp(-rng.random((10, S)) * 5)
    side = rng.integers(0, 3, S)
    w[:5] *= side != 1
    w[5:] *= side != 0
    return np.ascontiguousarray(w)


def _tss_ref(f, r, w):
    """oracle.reduce_np.tss_reduce of one gene; rows narrower than 4 features are tiled to 4 times
    their width first, so that numpy sums the shift axis in order as it does for 2002-wide rows."""
    from oracle.reduce_np import tss_reduce
    if f.shape[-1] >= 4:
        return tss_reduce(f, r, w)
    F = f.shape[-1]
    wide = tss_reduce(np.tile(f, (1, 4)), np.tile(r, (1, 4)), w).reshape(10, 4 * F)
    return np.ascontiguousarray(wide[:, :F]).reshape(-1)


@pytest.mark.parametrize("nfeat", [10, 37, 256, 257, 2002])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_shift_reduce_all_layouts(lib, flags, nfeat):
    """flags bit 0: the float64 fwd/rc average of test_shift_reduce_matches_numpy_bitwise, else
    the float32 0.5f*(a+b) of oracle.reduce_np.tss_reduce; bit 1: the legacy layout with a zero
    column ahead of each decay block.  nfeat 10 / 37: one partly filled workgroup; 256: exactly
    one; 257: the second workgroup has one live thread; S 1 / 8 / 9 / 13: the 8-shift load
    chunk's edges.  flags 0 must also equal features.tss_reduce (expecto_tss_reduce)."""
    from expecto_amd.features import tss_reduce
    rng = np.random.default_rng(60 + flags * 10 + nfeat)
    n = 3
    for S in (1, 8, 9, 13):
        fwd, rc, w = _signed(rng, (n, S, nfeat)), _signed(rng, (n, S, nfeat)), _masked_weights(rng, S)
        if flags & 1:
            preds = (fwd.astype(np.float64) + rc.astype(np.float64)) / 2
            want = np.sum(w[None, :, :, None] * preds[:, None, :, :], axis=2)
        else:
            want = np.stack([_tss_ref(fwd[g], rc[g], w) for g in range(n)]).reshape(n, 10, nfeat)
        if flags & 2:
            want = np.concatenate([np.zeros((n, 10, 1)), want], axis=2)
        want = np.ascontiguousarray(want.reshape(n, -1))
        out = Guarded(want.shape, np.float64)
        fd, rd, wd = dev(fwd), dev(rc), dev(w)
        st = lib.expecto_shift_reduce(P(fd), P(rd), P(wd), n, S, nfeat, flags, out.ptr, ST())
        assert st == 0, last_error(lib)
        got = out.result()
        assert_bits(got, want, f"shift_reduce flags {flags} nfeat {nfeat} S {S}")
        if flags == 0:
            assert_bits(got, tss_reduce(fd, rd, wd).cpu().numpy(), f"shift_reduce vs tss_reduce, S {S}")


def test_shift_reduce_refuses_bad_shapes(lib):
    rng = np.random.default_rng(61)
    fd, wd = dev(_signed(rng, (1, 2, 16))), dev(_masked_weights(rng, 2))
    out = Guarded((1, 10 * 17), np.float64)
    assert lib.expecto_shift_reduce(P(fd), P(fd), P(wd), 1, 2, 9, 0, out.ptr, ST()) == -1
    assert "bad shape" in last_error(lib)
    assert lib.expecto_shift_reduce(P(fd), P(fd), P(wd), 1, 2, 16, 4, out.ptr, ST()) == -1
    assert "bad flags" in last_error(lib)
    assert out.untouched()


@pytest.mark.parametrize("S", [1, 8, 9, 819])
@pytest.mark.parametrize("nfeat", [1, 2, 2050])
def test_tss_reduce_edges(lib, nfeat, S):
    """Host dispatch of expecto_tss_reduce: nfeat even, fwd and rc 8-byte aligned and out 16-byte
    aligned -> tss_reduce2_kernel (1024 pairs per workgroup: nfeat 2 is one pair, 2050 leaves the
    second workgroup one live thread); otherwise tss_reduce_kernel (nfeat 1, or `fwd` moved by
    4 bytes), which must give the same bits.  S = 819 fills the 64 KiB of LDS."""
    rng = np.random.default_rng(70 + nfeat + S)
    G = 2
    fwd, rc, w = _signed(rng, (G, S, nfeat)), _signed(rng, (G, S, nfeat)), _masked_weights(rng, S)
    want = np.stack([_tss_ref(fwd[g], rc[g], w) for g in range(G)])
    rd, wd = dev(rc), dev(w)
    results = []
    for off in (0, 4):
        fd = dev_offset(fwd, off)
        out = Guarded((G, 10 * nfeat), np.float64)
        assert out.ptr % 16 == 0 and fd.data_ptr() % 8 == off
        st = lib.expecto_tss_reduce(P(fd), P(rd), P(wd), G, S, nfeat, out.ptr, ST())
        assert st == 0, last_error(lib)
        results.append(out.result())
        assert_bits(results[-1], want, f"tss_reduce nfeat {nfeat} S {S} fwd offset {off}")
    assert_bits(results[0], results[1], "2-feature kernel vs scalar kernel")


def test_tss_reduce_refuses_820_shifts(lib):
    rng = np.random.default_rng(71)
    fd, wd = dev(_signed(rng, (1, 820, 2))), dev(_masked_weights(rng, 820))
    out = Guarded((1, 20), np.float64)
    assert lib.expecto_tss_reduce(P(fd), P(fd), P(wd), 1, 820, 2, out.ptr, ST()) == -1
    assert "n_shift <= 819" in last_error(lib)
    assert out.untouched()


# ---- variant reduction ---------------------------------------------------------------------

FAR = 1_000_000      # floor(|d| / 200) = 5000: exp(-0.2 * 5000) is 0 in float64, exp(-0.1 * 5000) is not
DISTS = [0, 199, -199, 200, -200, 201, -201, FAR, -FAR]
# (dist, strand_plus): every distance on both strands, and two fillers to make four calls of 5
VARIANTS = [(d, s) for s in (1, 0) for d in DISTS] + [(12345, 1), (-777, 0)]
SHIFTS9 = [0, -200, 200, -400, 400, -800, 800, -1600, 1600]


def _variant_inputs(rng, S, vs, nfeat):
    eff = _signed(rng, (S, len(vs), nfeat))
    dist = np.asarray([v[0] for v in vs], np.int64)
    plus = np.asarray([v[1] for v in vs], np.uint8)
    return eff, dist, plus


def _variant_call(lib, eff, dist, plus, shifts, lut, out_offset=0, eff_offset=0, use_lut_entry=True):
    S, n, nfeat = eff.shape
    ed = dev_offset(eff, eff_offset)
    dd, pd, sd = dev(dist), dev(plus), dev(np.asarray(shifts, np.int32))
    out = Guarded((n, 10 * nfeat), np.float64, offset=out_offset)
    if use_lut_entry:
        ld = None if lut is None else dev(lut)
        st = lib.expecto_variant_reduce_lut(P(ed), P(dd), P(pd), P(sd), S, n, nfeat, P(ld),
                                            0 if lut is None else lut.shape[1], out.ptr, ST())
    else:
        st = lib.expecto_variant_reduce(P(ed), P(dd), P(pd), P(sd), S, n, nfeat, out.ptr, ST())
    assert st == 0, last_error(lib)
    return out.result()


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("nfeat", [1, 2, 510, 512, 514])
def test_variant_reduce_lut_edges(lib, nfeat, S):
    """Host dispatch of expecto_variant_reduce_lut: nfeat even, effects 8-byte aligned, out
    16-byte aligned and at most 716 shifts -> variant_reduce_rows_kernel (256 pairs per
    workgroup: nfeat 2 is one pair, 510 / 512 end in and on the first workgroup, 514 leaves the
    second a single pair; `out` moved by 16 / 112 bytes changes the row stores' lead-in); above
    716 shifts variant_reduce2_kernel (test_variant_features_past_the_row_kernels_lds); nfeat
    odd or `effects` moved by 4 bytes -> variant_reduce_kernel, the same bits.  Distances 0,
    +-199, +-200, +-201 (d = 0 counts on both sides, the floor's steps) and +-1,000,000 (the
    0.2 decay is exactly 0, the others are not) on both strands, in calls of 5 and of 1."""
    from expecto_amd.features import decay_table
    from oracle.reduce_np import variant_reduce, variant_weights
    rng = np.random.default_rng(80 + nfeat + S)
    shifts = SHIFTS9[:S]
    groups = [VARIANTS[i:i + 5] for i in range(0, 20, 5)] + [[v] for v in VARIANTS[:18:3]]
    for gi, vs in enumerate(groups):
        eff, dist, plus = _variant_inputs(rng, S, vs, nfeat)
        lut = decay_table(dist, plus, shifts)
        want = variant_reduce(list(eff), variant_weights(dist, plus.astype(bool), shifts), nfeat)
        got = _variant_call(lib, eff, dist, plus, shifts, lut, out_offset=(0, 16, 112)[gi % 3])
        assert_bits(got, want, f"variant_reduce_lut nfeat {nfeat} S {S} variants {vs}")
        if gi == 0:
            scalar = _variant_call(lib, eff, dist, plus, shifts, lut, eff_offset=4)
            assert_bits(scalar, got, "scalar kernel (effects off 8 bytes) vs aligned run")


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("nfeat", [2, 37])
def test_variant_reduce_device_exp(lib, nfeat, S):
    """The device exp: expecto_variant_reduce (no table) and expecto_variant_reduce_lut with a
    table of length 1 holding 2.0 in place of exp(0), so every floor(|d|/200) >= 1 falls through
    to the device and a weight still read from the table stands out.  Variants whose shifts all
    have floor >= 1 must agree bitwise between the two runs.  Against the float64 oracle each
    output lies within 4 * 2^-52 * sum_j |eff_j| * W_j (1 ulp for the device exp, 1 for the
    product, the rest for the nine sums); the table run is held to the oracle with 2.0 put in
    place of exp(0).  nfeat 2: the row-staged kernel; 37: the scalar kernel.
    Worst observed |error| / bar on an MI355X: 0.40 (nfeat 37, S 9; 0.19 to 0.40 over the four cases)."""
    from oracle.reduce_np import variant_reduce, variant_weights
    rng = np.random.default_rng(90 + nfeat + S)
    shifts = SHIFTS9[:S]
    eff, dist, plus = _variant_inputs(rng, S, VARIANTS, nfeat)
    no_table = _variant_call(lib, eff, dist, plus, shifts, None, use_lut_entry=False)
    wrong = np.full((5, 1), 2.0)
    short = _variant_call(lib, eff, dist, plus, shifts, wrong)
    sgn = np.where(plus.astype(bool), 1, -1)
    fl = np.floor(np.abs(dist[:, None] * sgn[:, None] + np.asarray(shifts)[None, :] * sgn[:, None]) / 200.0)
    device_only = (fl >= 1).all(axis=1)
    assert device_only.sum() >= 4 and (~device_only).sum() >= 4
    assert_bits(short[device_only], no_table[device_only], "length-1 table vs no table where fl >= 1")
    weights = variant_weights(dist, plus.astype(bool), shifts)
    tabled = [np.where((fl[:, j] == 0)[:, None], 2.0 * w, w) for j, w in enumerate(weights)]
    worst = 0.0
    for name, got, ws in (("no table", no_table, weights), ("length-1 table", short, tabled)):
        want = variant_reduce(list(eff), ws, nfeat)
        bar = 4 * 2.0 ** -52 * variant_reduce(list(np.abs(eff)), ws, nfeat)
        err = np.abs(got - want)
        ratio = np.divide(err, bar, out=np.where(err > 0, np.inf, 0.0), where=bar > 0)
        print(f"device exp, {name}, nfeat {nfeat} S {S}: worst |error| / bar = {ratio.max():.4f}")
        worst = max(worst, float(ratio.max()))
        assert (err <= bar).all(), f"{name}: worst |error| / bar = {ratio.max():.3f}"
    assert np.isfinite(worst)


# ---- gblinear scoring ----------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_gblinear_predict_edges(lib, n):
    """Rows 1 / 63 / 64 / 65 / 130 around the 64-row workgroup, columns 0 / 1 / 63 / 64 / 65 / 200
    around the 64-column slab; X is a column slice of a wider float64 matrix (ld 300 > its 280
    columns), the column map unsorted with repeats, values that round when cast to float32."""
    from oracle.gblinear_np import predict
    rng = np.random.default_rng(95 + n)
    W, c0, width = 300, 3, 280
    full = rng.standard_normal((n, W))
    special = np.array([1 + 2.0 ** -30, 1 - 2.0 ** -30, 2.0 ** -140, 1e-50, -0.0, 3.0000000001, -(1 + 2.0 ** -24)])
    full[rng.integers(0, n, 40), rng.integers(0, W, 40)] = special[rng.integers(0, special.size, 40)]
    full[0, c0:c0 + special.size] = special
    Xd = dev(full)
    bias, base = 0.37, 0.5
    init = np.float32(np.float32(bias) + np.float32(base))
    for ncols in (0, 1, 63, 64, 65, 200):
        cols = rng.integers(0, width, ncols).astype(np.int32)
        k = min(ncols, special.size)
        cols[:k] = np.arange(special.size)[::-1][:k]            # row 0's planted values, in descending order
        if ncols >= 10:
            cols[-1], cols[-2] = cols[0], cols[-3]              # repeats, next to each other and far apart
            assert (np.diff(cols) < 0).any() and len(set(cols.tolist())) < ncols
        w = rng.standard_normal(ncols).astype(np.float32)
        out = Guarded((n,), np.float32)
        cd, wd = (dev(cols), dev(w)) if ncols else (None, None)
        st = lib.expecto_gblinear_predict(Xd.data_ptr() + 8 * c0, n, W, P(cd), ncols, P(wd), float(init),
                                          out.ptr, ST())
        assert st == 0, last_error(lib)
        got = out.result()
        want = predict(full[:, c0:c0 + width][:, cols], w, bias, base)
        assert_bits(got, want, f"gblinear n {n} ncols {ncols}")
        if ncols == 0:
            assert_bits(got, np.full(n, init, np.float32), "init alone")
