"""numpy restatement of the empirical significance step (include/expecto_hip.h, "Empirical
significance"): tail counts by ``np.searchsorted``, the host table of ``-log10 e``, and the
per-variant summaries with the sum in the order S (``contrib_ref.wave_sum``).  Used by
tests/test_ecdf_ref.py, tests/test_ecdf_host.py, tests/test_gpu_ecdf.py and
tests/test_gpu_significance.py; it also builds the backgrounds and queries those tests share."""
import numpy as np

from contrib_ref import wave_sum


def tail_counts(bg, x, cols):
    """bg [C, B] f32 ascending per row; x [n, >= max(cols) + 1] f32; cols ascending mark indices.
    int32 [n, nc]: the number of bg[cols[j]] values >= |x[v, cols[j]]|, -1 for a NaN query."""
    bg, x = np.asarray(bg, np.float32), np.asarray(x, np.float32)
    cols = np.asarray(cols, np.int64)
    B = bg.shape[1]
    a = np.abs(x[:, cols])
    ge = np.empty(a.shape, np.int32)
    for j, c in enumerate(cols):
        ge[:, j] = B - np.searchsorted(bg[c], a[:, j], side="left")
    ge[np.isnan(a)] = -1
    return ge


def lut(B):
    """float64 [B + 1]: lut[k] = -log10((k + 1) / (B + 1))."""
    return -np.log10((np.arange(B + 1, dtype=np.float64) + 1.0) / (B + 1.0))


def k_alpha(alpha, B):
    return int(np.floor(alpha * (B + 1)))


def evalues(ge, B):
    """float64 (ge + 1) / (B + 1); NaN where ge is -1."""
    e = (ge.astype(np.float64) + 1.0) / (B + 1.0)
    e[ge < 0] = np.nan
    return e


def summaries(ge, table, k_a):
    """(mean_nlog f64, max_nlog f64, top i32, n_sig i32) per row of ge [n, nc]; a row holding a -1
    gets NaN, NaN, -1, -1."""
    ge = np.asarray(ge, np.int32)
    n, nc = ge.shape
    bad = (ge < 0).any(1)
    nlog = table[np.maximum(ge, 0)]
    mean = wave_sum(nlog) / float(nc)
    mx = nlog.max(1)
    top = np.argmin(ge, 1).astype(np.int32)            # the first of the smallest counts
    n_sig = (ge.astype(np.int64) + 1 <= k_a).sum(1).astype(np.int32)
    mean[bad], mx[bad], top[bad], n_sig[bad] = np.nan, np.nan, -1, -1
    return mean, mx, top, n_sig


# ---------------------------------------------------------------------------- shared test inputs
def background(C, B, seed):
    """[C, B] f32 ascending rows of magnitudes with runs of equal values (the rows are drawn from
    about B / 3 distinct values), a zero, a denormal and, in every second row, +inf at the end."""
    rng = np.random.default_rng(seed)
    pool = np.abs(rng.normal(0, 0.05, (C, max(1, B // 3)))).astype(np.float32)
    bg = np.take_along_axis(pool, rng.integers(0, pool.shape[1], (C, B)), 1)
    if B >= 4:
        bg[:, 0] = 0.0
        bg[:, 1] = np.float32(1e-41)
        bg[1::2, 2] = np.inf
    bg.sort(1)
    return bg


def queries(bg, n, stride, seed):
    """[n, stride] f32 (stride >= C; the columns past C hold NaN): per column a cycle of exact
    background values with either sign, midpoints of neighbours, values below the minimum and above
    the maximum, +-0.0, denormals, +-inf and random draws."""
    rng = np.random.default_rng(seed)
    C, B = bg.shape
    x = np.full((n, stride), np.nan, np.float32)
    idx = rng.integers(0, B, (n, C))
    exact = bg.T[idx, np.arange(C)[None, :]]
    nxt = bg.T[np.minimum(idx + 1, B - 1), np.arange(C)[None, :]]
    finite = np.where(np.isfinite(bg), bg, 0)
    with np.errstate(all="ignore"):
        mid = ((exact.astype(np.float64) + nxt) / 2).astype(np.float32)
    kinds = [exact, -exact, mid, np.broadcast_to(bg[:, 0] / np.float32(2), (n, C)),
             np.broadcast_to(finite.max(1) * 2 + 1, (n, C)), np.zeros((n, C), np.float32),
             np.full((n, C), -0.0, np.float32), np.full((n, C), 1e-41, np.float32), np.full((n, C), -3e-45, np.float32),
             np.full((n, C), np.inf, np.float32), np.full((n, C), -np.inf, np.float32),
             rng.normal(0, 0.05, (n, C)).astype(np.float32)]
    pick = (np.arange(n)[:, None] + np.arange(C)[None, :]) % len(kinds)
    vals = np.choose(pick, kinds)
    x[:, :C] = vals
    return x
