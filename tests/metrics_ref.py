"""numpy restatements of the metric kernels (include/expecto_hip.h: expecto_rank2_*, expecto_model_metrics,
expecto_bootstrap_coef_stats), shared by test_metrics_ref.py (which anchors them to scipy / sklearn / numpy
through tests/golden/metrics/values.json) and test_gpu_metrics.py (which holds the kernels to them bit for
bit), and the seeded inputs both use."""
import numpy as np

THREADS = 256


def rank2_ref(x):
    """Doubled average ranks by the counting definition: 2 #{x_j < x_i} + #{x_j == x_i} + 1 (int32)."""
    x = np.asarray(x)
    out = np.empty(x.shape[0], np.int32)
    for i0 in range(0, x.shape[0], 2048):                 # a block of i at a time keeps the table small
        xi = x[i0:i0 + 2048, None]
        with np.errstate(invalid="ignore"):
            out[i0:i0 + 2048] = 2 * (x[None, :] < xi).sum(1) + (x[None, :] == xi).sum(1) + 1
    return out


def spearman_ref(a, b):
    """rho from Python-int sums of the doubled ranks a, b."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    n = len(a)
    sa, sb = sum(a), sum(b)
    sab = sum(p * q for p, q in zip(a, b))
    saa, sbb = sum(p * p for p in a), sum(q * q for q in b)
    num, da, db = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    assert max(abs(num), da, db) < 2 ** 63
    den = np.sqrt(np.float64(float(da)) * np.float64(float(db)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(float(num)) / den


def tree_sum(v):
    """The device's float64 sum: thread t adds elements t, t+256, ... in ascending order onto +0.0, then the
    256 partials fold by p[i] = p[i] + p[i+w], w = 128 ... 1."""
    v = np.asarray(v, np.float64)
    p = np.zeros(THREADS)
    for k in range(0, v.shape[0], THREADS):
        c = v[k:k + THREADS]
        p[:c.shape[0]] = p[:c.shape[0]] + c
    w = THREADS // 2
    while w >= 1:
        p[:w] = p[:w] + p[w:2 * w]
        w //= 2
    return p[0]


def pearson_r2_ref(pred, y):
    """(pearson, r2) in float64, two passes, in the device's order; pred is float32, widened exactly."""
    x, y = np.asarray(pred, np.float32).astype(np.float64), np.asarray(y, np.float64)
    n = np.float64(x.shape[0])
    with np.errstate(all="ignore"):
        mx, my = tree_sum(x) / n, tree_sum(y) / n
        dx, dy, e = x - mx, y - my, y - x
        sxy, sxx, syy, ssr = tree_sum(dx * dy), tree_sum(dx * dx), tree_sum(dy * dy), tree_sum(e * e)
        r = sxy / np.sqrt(sxx * syy)
        if r > 1.0:
            r = np.float64(1.0)
        if r < -1.0:
            r = np.float64(-1.0)
        r2 = np.float64(1.0) - ssr / syy
        if syy == 0.0:
            r2 = np.float64(1.0 if ssr == 0.0 else 0.0)
    return r, r2


def model_metrics_ref(pred, y):
    """[P, 3] (pearson, spearman, r2); y [n] or [P, n].  A NaN in a model's pred or y gives three NaNs."""
    pred = np.atleast_2d(np.asarray(pred, np.float32))
    y = np.asarray(y, np.float64)
    out = np.empty((pred.shape[0], 3))
    ry = rank2_ref(y) if y.ndim == 1 else None
    for m in range(pred.shape[0]):
        ym = y if y.ndim == 1 else y[m]
        if np.isnan(pred[m]).any() or np.isnan(ym).any():
            out[m] = np.nan
            continue
        r, r2 = pearson_r2_ref(pred[m], ym)
        out[m] = r, spearman_ref(rank2_ref(pred[m]), ry if ry is not None else rank2_ref(ym)), r2
    return out


def coef_stats_ref(W, w_main):
    """mean, se, z, cv per coefficient: the B models walked in ascending order."""
    W, w_main = np.asarray(W, np.float64), np.asarray(w_main, np.float64)
    B = W.shape[0]
    s = np.zeros(W.shape[1])
    for b in range(B):
        s = s + W[b]
    mean = s / np.float64(B)
    q = np.zeros(W.shape[1])
    for b in range(B):
        d = W[b] - mean
        q = q + d * d
    with np.errstate(divide="ignore", invalid="ignore"):
        se = np.sqrt(q / np.float64(B - 1))
        return {"mean": mean, "se": se, "z": w_main / se, "cv": se / np.abs(mean)}


def zscore_order(z):
    """Row order of input_features_sorted_by_zscore.csv: |z| descending, ties to the lower row, NaN last."""
    return np.argsort(-np.abs(np.asarray(z, np.float64)), kind="stable")


def extended(pred, y):
    """(pearson, r2) by the textbook formulas in np.longdouble."""
    x, t = np.asarray(pred).astype(np.longdouble), np.asarray(y).astype(np.longdouble)
    dx, dy = x - x.mean(), t - t.mean()
    return (dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum()), 1 - ((t - x) ** 2).sum() / (dy * dy).sum()


def library_errors(golden_pairs):
    """(pearson, r2): the largest |scipy / sklearn - extended precision| over the golden pair cases, the
    reference libraries' own rounding.  Four times these are the bars a float64 Pearson / R2 is held to."""
    ep = er = 0.0
    for g in golden_pairs:
        xp, xr = extended(*pair_case(g["n"], g["ties"]))
        ep = max(ep, abs(float(np.longdouble(g["pearsonr"]) - xp)))
        er = max(er, abs(float(np.longdouble(g["r2_score"]) - xr)))
    return ep, er


# -- seeded inputs of the golden file ---------------------------------------------------------------------------
PAIR_CASES = [(37, False), (37, True), (1003, False), (1003, True), (4099, False), (4099, True), (24576, False),
              (24576, True)]
STATS_CASES = [(2, 1), (3, 257), (800, 1000)]


def pair_case(n, ties, seed=0):
    """(pred float32 [n], y float64 [n]): a noisy linear relation; ``ties`` rounds both to a coarse grid."""
    rng = np.random.default_rng([seed, n, int(ties)])
    y = rng.standard_normal(n) * 2.0 + 1.0
    pred = 0.6 * y + rng.standard_normal(n) + 0.5
    if ties:
        y, pred = np.round(y * 4.0) / 4.0, np.round(pred * 2.0) / 2.0
    return pred.astype(np.float32), y


def stats_case(B, F, seed=0):
    """(W float64 [B, F], w_main float64 [F]) at the %g precision of a model dump."""
    rng = np.random.default_rng([seed, B, F])
    W = rng.standard_normal((B, F)) * rng.uniform(1e-4, 0.1, F) + rng.standard_normal(F) * 0.05
    g = np.vectorize(lambda v: float("%g" % v))
    return g(W), g(rng.standard_normal(F) * 0.05)
