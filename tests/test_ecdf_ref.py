"""CPU: the numpy restatement of the empirical significance step (tests/ecdf_ref.py) against
brute-force counting on tiny inputs, and the order S it imports against a literal expansion."""
import numpy as np

import ecdf_ref
from contrib_ref import wave_sum


def _brute(bg, x, cols):
    n, nc = x.shape[0], len(cols)
    ge = np.empty((n, nc), np.int32)
    for v in range(n):
        for j, c in enumerate(cols):
            a = abs(float(x[v, c]))
            ge[v, j] = -1 if a != a else sum(1 for b in bg[c] if float(b) >= a)
    return ge


def test_tail_counts_equal_brute_force_counting():
    for C, B, seed in ((1, 1, 0), (3, 2, 1), (4, 7, 2), (5, 33, 3)):
        bg = ecdf_ref.background(C, B, seed)
        assert (np.diff(bg, axis=1) >= 0).all()
        x = ecdf_ref.queries(bg, 29, C + 2, seed + 10)
        x[3, 0] = np.nan
        cols = np.arange(C)[::2] if C > 2 else np.arange(C)
        got = ecdf_ref.tail_counts(bg, x, cols)
        assert got.dtype == np.int32 and np.array_equal(got, _brute(bg, x, cols))
        assert got[3, 0] == -1 and got.max() <= B and (np.delete(got.ravel(), 3 * len(cols)) >= 0).all()


def test_ties_and_infinities_count():
    bg = np.array([[0.0, 1.0, 1.0, 1.0, 2.0, np.inf, np.inf]], np.float32)
    x = np.array([[1.0], [-1.0], [1.5], [np.inf], [-np.inf], [0.0], [-0.0], [3.0], [np.nan]], np.float32)
    assert ecdf_ref.tail_counts(bg, x, [0])[:, 0].tolist() == [6, 6, 3, 2, 2, 7, 7, 2, -1]


def test_table_and_evalues():
    B = 9
    t = ecdf_ref.lut(B)
    assert t.shape == (10,) and t.dtype == np.float64
    assert t[B] == 0.0 and t[0] == 1.0 and (np.diff(t) < 0).all()
    ge = np.array([[0, 9, -1]], np.int32)
    e = ecdf_ref.evalues(ge, B)
    assert e[0, 0] == 0.1 and e[0, 1] == 1.0 and np.isnan(e[0, 2])
    assert [ecdf_ref.k_alpha(a, B) for a in (0.0, 0.05, 0.1, 0.25, 1.0)] == [0, 0, 1, 2, 10]


def test_summaries_by_hand():
    B = 99
    t = ecdf_ref.lut(B)
    ge = np.array([[5, 0, 7, 0], [99, 99, 99, 99], [3, -1, 0, 2]], np.int32)
    mean, mx, top, n_sig = ecdf_ref.summaries(ge, t, k_a=1)
    assert top.tolist() == [1, 0, -1] and n_sig.tolist() == [2, 0, -1]
    assert mx[0] == t[0] == 2.0 and mx[1] == 0.0 and np.isnan(mx[2]) and np.isnan(mean[2])
    assert mean[0] == (((t[5] + t[7]) + (t[0] + t[0])) / 4.0) and mean[1] == 0.0
    assert ecdf_ref.summaries(ge[:2], t, k_a=B + 1)[3].tolist() == [4, 4]
    assert ecdf_ref.summaries(ge[:2], t, k_a=0)[3].tolist() == [0, 0]


def _literal(x):
    """S written out: 64 strided sums left to right from -0.0, folded 32 .. 1."""
    p = [-0.0] * 64
    for i, v in enumerate(x):
        p[i % 64] = p[i % 64] + float(v)
    s = 32
    while s:
        for l in range(s):
            p[l] = p[l] + p[l + s]
        s //= 2
    return p[0]


def test_wave_sum_is_the_literal_order():
    rng = np.random.default_rng(4)
    for c in (1, 2, 63, 64, 65, 130, 2002):
        x = rng.normal(0, 1, c) * 10.0 ** rng.integers(-8, 8, c)
        assert wave_sum(x[None])[0].tobytes() == np.float64(_literal(x)).tobytes(), c
    assert wave_sum(np.zeros((1, 0)))[0] == 0.0
