"""Host-side geometry of the segment path's pool2 and of its alt runs (beluga.hip seg_delta_table,
seg_delta_pool, pool2_tile_seams; gemm_kernel.h epilogue_pool_ph02), without a GPU.

* seg_delta_table restated for any list of pool2 phases: every run it places stays inside its layer
  (phase-0 geometry), and covers every row of the layer that an SNV at q changes -- the property the
  alt runs rely on -- for every phase, every phase subset and every segment length residue mod 16.
* The fused conv4 + pool2 epilogue (phases {0, 2}): the alt windows' ref conv4 rows that it keeps
  unpooled fit the 32-row-per-segment buffer for every SNV position; the 4-aligned conv3 stride
  puts every segment's pool groups on 4-aligned rows of conv4's M index space; pool2_tile_seams
  writes exactly the valid phase-2 groups that straddle two 256-row tiles, each once."""
import itertools

import numpy as np
import pytest

K_DW = (0, 8, 5, 12, 6, 13, 20)   # kDW: rows of the alt run of conv1, conv2 + pool1, conv3, pool2, conv5, conv6
K_DW4 = K_DW[4]    # kDW[4]: pooled rows of an alt run per phase
K_W4U = 19         # kW4u: conv4 rows of the alt run
K_SEG_EDGE = 32    # kSegEdge

SMALL_L = (2000, 2004, 2008, 2012, 2204, 2212, 2220, 3600)
LARGE_L = (41_800, 41_804, 41_808, 41_812)
PHASE_SETS = [s for n in range(1, 5) for s in itertools.combinations(range(4), n)]


def floor4(v):
    return v >> 2 if v >= 0 else -((3 - v) >> 2)


def clampi(v, lo, hi):
    return max(lo, min(v, hi))


def seg_dims(L):
    T1 = L - 7
    P1 = (T1 - 7) // 4
    T3 = P1 - 7
    T4 = T3 - 7
    S5 = T4 // 4
    return T1, P1, T3, T4, S5


def edge_range(q, L):
    """[lo, hi) of conv4 rows seg_delta_pool reads for an SNV at q (beluga.hip seg_delta_table)."""
    T1, P1, T3, T4, S5 = seg_dims(L)
    r1 = clampi(q - 7, 0, T1 - 8)
    r2 = clampi(floor4(r1 - 7), 0, P1 - 5)
    r3 = clampi(r2 - 7, 0, T3 - 12)
    r4 = clampi(r3 - 7, 0, T4 - K_W4U)
    t5 = clampi(floor4(r4 - 0), 0, S5 - K_DW4)
    t6 = clampi(floor4(r4 - 2), 0, S5 - K_DW4)
    lo = min(4 * t5, 2 + 4 * t6)
    hi = max(4 * (t5 + K_DW4), 2 + 4 * (t6 + K_DW4))
    return lo, hi, t5, t6


@pytest.mark.parametrize("L", [41_800, 3_600, 10_000, 41_804, 41_808, 41_812, 2_000, 2_004, 2_008, 2_012, 2_212, 2_220])
def test_alt_edge_rows_fit_the_segment_buffer(L):
    for q in range(0, L, 3):
        lo, hi, t5, t6 = edge_range(q, L)
        assert 0 <= lo < hi and hi - lo <= K_SEG_EDGE, (L, q, lo, hi)
        # every row seg_delta_pool reads (phase p, pooled rows tab[5 + i] .. + 6, 4 rows each) is inside
        for p, t in ((0, t5), (2, t6)):
            rows = [p + 4 * (t + g) + j for g in range(K_DW4) for j in range(4)]
            assert lo <= min(rows) and max(rows) < hi


@pytest.mark.parametrize("L", [41_800, 41_804, 41_808, 41_812, 3_600])
def test_segment_rows_start_4_aligned_with_the_padded_conv3_stride(L):
    _, _, T3, T4, _ = seg_dims(L)
    t3p = (T3 + 3) & ~3
    assert t3p % 4 == 0 and T4 <= t3p < T3 + 4
    starts = np.arange(64) * t3p
    assert np.all(starts % 4 == 0)
    # a phase-0 group (rows t .. t+3, t = 0 mod 4 in segment coordinates) is one lane's 4 accumulator
    # rows of a 16-row block; a phase-2 group crosses to the next lane group or block
    for w in range(8):
        for t in range(0, T4 - 3, 4):
            m = w * t3p + t
            assert m % 4 == 0 and (m % 16) // 4 == ((m + 3) % 16) // 4


# ---- seg_delta_table for any phase list -------------------------------------------------------------

def seg_delta_table(L, q, phases):
    """The kSegTab ints seg_delta_table (beluga.hip) writes for an SNV at base q (an int array: one
    table per q) of a segment of L bases in the strand's orientation, for the phases `phases` in
    ascending order: q, r1, r2, r3, r4u, then r4p, r5, r6 per phase index (t[5 + i], t[9 + i],
    t[13 + i]).  The arithmetic is the kernel's, on arrays."""
    T1, P1, T3, T4, S5 = seg_dims(L)
    T5, T6 = S5 - 7, S5 - 14
    q = np.asarray(q, np.int64)
    t = np.zeros((20, q.size), np.int64)
    r1 = np.clip(q - 7, 0, T1 - K_DW[1])
    r2 = np.clip((r1 - 7) >> 2, 0, P1 - K_DW[2])        # >> on int64 floors, as floor4 does
    r3 = np.clip(r2 - 7, 0, T3 - K_DW[3])
    r4 = np.clip(r3 - 7, 0, T4 - K_W4U)
    t[0], t[1], t[2], t[3], t[4] = q, r1, r2, r3, r4
    for i, p in enumerate(phases):
        r4p = np.clip((r4 - p) >> 2, 0, S5 - K_DW[4])
        r5 = np.clip(r4p - 7, 0, T5 - K_DW[5])
        t[5 + i], t[9 + i], t[13 + i] = r4p, r5, np.clip(r5 - 7, 0, T6 - K_DW[6])
    return t


def test_floor4_is_the_shift():
    v = np.arange(-40, 40)
    assert [floor4(int(x)) for x in v] == list(v >> 2) == [int(x) // 4 for x in v]


class _Rows:
    """Inclusive row ranges [lo, hi] per q; `on` marks the q whose range is not empty."""

    def __init__(self, lo, hi, on=None):
        self.lo, self.hi = lo, hi
        self.on = (lo <= hi) if on is None else (on & (lo <= hi))

    def conv(self, t_valid):
        """Rows of an 8-tap layer with t_valid rows that read one of these rows."""
        return _Rows(np.maximum(self.lo - 7, 0), np.minimum(self.hi, t_valid - 1), self.on)

    def pool(self, p, n_valid):
        """Pooled rows g < n_valid (rows p + 4 g .. p + 4 g + 3) that hold one of these rows."""
        return _Rows(np.maximum((self.lo - p) >> 2, 0), np.minimum((self.hi - p) >> 2, n_valid - 1), self.on)

    def inside(self, r, w):
        """Every non-empty range lies in the run [r, r + w)."""
        return bool(np.all(~self.on | ((r <= self.lo) & (self.hi < r + w))))


def _q_of(L):
    return np.arange(0, L, 1 if L in SMALL_L else 3)


@pytest.mark.parametrize("L", SMALL_L + LARGE_L)
def test_alt_runs_stay_inside_their_layers(L):
    """Table bounds, for every phase subset: the run of every layer lies in the layer's rows (the
    phase-0 geometry S5, T5, T6 the ref blocks are laid out with)."""
    T1, P1, T3, T4, S5 = seg_dims(L)
    T5, T6 = S5 - 7, S5 - 14
    assert T6 >= 106 and (L > 2000 or T6 == 106)
    q = _q_of(L)
    for phases in PHASE_SETS:
        t = seg_delta_table(L, q, phases)
        assert np.all((0 <= t[1]) & (t[1] + K_DW[1] <= T1)) and np.all((0 <= t[2]) & (t[2] + K_DW[2] <= P1))
        assert np.all((0 <= t[3]) & (t[3] + K_DW[3] <= T3)) and np.all((0 <= t[4]) & (t[4] + K_W4U <= T4))
        for i in range(len(phases)):
            r4p, r5, r6 = t[5 + i], t[9 + i], t[13 + i]
            assert np.all((0 <= r4p) & (r4p + K_DW[4] <= S5)), (L, phases, i)
            assert np.all((0 <= r5) & (r5 + K_DW[5] <= T5)), (L, phases, i)
            assert np.all((0 <= r6) & (r6 + K_DW[6] <= T6)), (L, phases, i)
        assert not t[5 + len(phases):9].any() and not t[13 + len(phases):17].any()   # unused phase slots


@pytest.mark.parametrize("L", SMALL_L + LARGE_L)
def test_alt_runs_cover_every_changed_row(L):
    """Coverage, for every phase subset: the rows of every layer that an SNV at q changes (by the
    receptive field: 8 taps, pool 4, 8 taps, 8 taps, pool 4 at phase p, 8 taps, 8 taps; clipped to the
    layer's valid rows, a phase p block holding (T4 - p) // 4 pooled rows) lie in the layer's run.  And
    run by run, as the kernels chain them: every valid row that reads a row of the previous run lies in
    its own run, so a row outside the runs sees ref operands only."""
    T1, P1, T3, T4, S5 = seg_dims(L)
    q = _q_of(L)
    snv = _Rows(q, q)
    c1 = snv.conv(T1)
    c2 = c1.conv(T1 - 7)
    p1 = c2.pool(0, P1)
    c3 = p1.conv(T3)
    c4 = c3.conv(T4)
    for phases in PHASE_SETS:
        t = seg_delta_table(L, q, phases)
        assert c1.on.all() and c1.inside(t[1], K_DW[1])
        assert p1.inside(t[2], K_DW[2]) and c3.inside(t[3], K_DW[3]) and c4.inside(t[4], K_W4U)
        # run by run below pool1: conv1 rows of the run feed pooled rows [r2, r2 + 5), and so on down
        assert _Rows(t[1], t[1] + K_DW[1] - 1).conv(T1 - 7).pool(0, P1).inside(t[2], K_DW[2])
        assert _Rows(t[2], t[2] + K_DW[2] - 1).conv(T3).inside(t[3], K_DW[3])
        assert _Rows(t[3], t[3] + K_DW[3] - 1).conv(T4).inside(t[4], K_W4U)
        for i, p in enumerate(phases):
            sp = (T4 - p) // 4           # valid pooled rows of phase p: p + 4 g + 3 < T4
            assert sp in (S5 - 1, S5)
            r4p, r5, r6 = t[5 + i], t[9 + i], t[13 + i]
            g = c4.pool(p, sp)
            c5 = g.conv(sp - 7)
            c6 = c5.conv(sp - 14)
            what = (L, phases, p)
            assert g.inside(r4p, K_DW[4]), what
            assert c5.inside(r5, K_DW[5]), what
            assert c6.inside(r6, K_DW[6]), what
            assert _Rows(t[4], t[4] + K_W4U - 1).pool(p, sp).inside(r4p, K_DW[4]), what
            assert _Rows(r4p, r4p + K_DW[4] - 1).conv(sp - 7).inside(r5, K_DW[5]), what
            assert _Rows(r5, r5 + K_DW[5] - 1).conv(sp - 14).inside(r6, K_DW[6]), what
            if L in SMALL_L:   # the changed rows by enumeration, for a few q, against the interval form
                for k in (0, 7, 8, L // 2, L - 2001, L - 2000, 1999, 2000 if L > 2000 else 1000, L - 9, L - 1):
                    # conv4 row r reads bases 4 r .. 4 r + 73 (7 + 7 + 3, then 4 x (7 + 7))
                    rows4 = {r for r in range(T4) if 4 * r <= k <= 4 * r + 73}
                    gs = {x for x in range(sp) if rows4 & set(range(p + 4 * x, p + 4 * x + 4))}
                    assert (min(gs), max(gs)) == (g.lo[k], g.hi[k]) if gs else not g.on[k], (what, k)


def test_coverage_check_is_not_vacuous():
    """The coverage check above fails for a table off by one phase: phase p's pooled run taken with
    phase p + 1's start misses a changed row for some q."""
    L = 2204
    T1, P1, T3, T4, S5 = seg_dims(L)
    q = _q_of(L)
    c4 = _Rows(q, q).conv(T1).conv(T1 - 7).pool(0, P1).conv(T3).conv(T4)
    t = seg_delta_table(L, q, (0, 1, 2, 3))
    missed = [not c4.pool(p, (T4 - p) // 4).inside(t[5 + (i + 3) % 4], K_DW[4]) for i, p in enumerate((0, 1, 2, 3))]
    assert any(missed), missed


# ---- pool2_tile_seams --------------------------------------------------------------------------------

def tile_seam_groups(n_seg, s_in, t4, margin=3):
    """(segment, pooled row) of the phase-2 rows pool2_tile_seams (beluga.hip) writes for a fused
    conv4 + pool2 launch over n_seg segment blocks of s_in rows, t4 of them valid: one workgroup per
    boundary b = 256 k between two of the launch's 256-row tiles.  (margin: the kernel's 3.)"""
    M = n_seg * s_in
    m_tiles = (M + 255) // 256
    out = []
    for k in range(1, m_tiles):
        b = 256 * k
        if b + 1 >= M:
            continue
        w = (b - 2) // s_in
        t = b - 2 - w * s_in
        if t + margin >= t4:
            continue
        assert t >= 2 and (t - 2) % 4 == 0, (k, t)   # a phase-2 group: its pooled index (t - 2) >> 2 is exact
        out.append((w, (t - 2) >> 2))
    return out


def straddling_phase2_groups(n_seg, s_in, t4):
    """By enumeration: the valid phase-2 groups (rows 2 + 4 g .. 5 + 4 g < t4 of a segment) whose four
    rows lie in two 256-row tiles of the launch's n_seg * s_in rows."""
    out = []
    for w in range(n_seg):
        for g in range(t4 // 4 + 1):
            m = w * s_in + 2 + 4 * g     # its conv4 rows m .. m + 3 of the launch
            if 2 + 4 * g + 3 < t4 and m // 256 != (m + 3) // 256:
                out.append((w, g))
    return out


@pytest.mark.parametrize("L", SMALL_L + LARGE_L)
def test_tile_seams_are_the_straddling_phase2_groups(L):
    _, _, T3, T4, S5 = seg_dims(L)
    s_in = (T3 + 3) & ~3
    want = straddling_phase2_groups(8, s_in, T4)
    got = tile_seam_groups(8, s_in, T4)
    assert len(set(got)) == len(got)                       # each written once
    assert sorted(got) == want, (L, s_in, T4)
    assert want and all(g < (T4 - 2) // 4 <= S5 for _, g in got)


def test_tile_seam_rule_is_tight():
    """Boundaries in a segment's rows past its valid ones are skipped for some of the lengths, and the
    skip test one row wider (t + 4 >= t4) would drop a valid group: the group that ends on the
    segment's last valid row, which exists only for T4 % 4 == 2 (L % 16 == 0)."""
    skipped = lost = 0
    for L in SMALL_L + LARGE_L:
        _, _, T3, T4, _ = seg_dims(L)
        s_in = (T3 + 3) & ~3
        for n_seg in range(2, 40):
            want = straddling_phase2_groups(n_seg, s_in, T4)
            tiles = (n_seg * s_in + 255) // 256
            skipped += len(want) < tiles - 1
            wide = tile_seam_groups(n_seg, s_in, T4, margin=4)
            assert set(wide) <= set(want)
            if len(wide) < len(want):
                assert T4 % 4 == 2
                lost += 1
    assert skipped and lost
