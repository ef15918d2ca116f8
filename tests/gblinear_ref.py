"""numpy restatements of the gblinear training steps (DESIGN.md "Training gblinear models"),
shared by test_train_host.py and test_gpu_train.py.

``train_ref(..., f32=True)`` is R32: float32 state, every float32 product and sum rounded on its
own, the sums over rows in double -- the steps exactly as written.  ``f32=False`` is R64: the
same steps with float64 for everything.  ``noise = max|R32 - R64|`` over ``[w; b]`` is the size
of R32's own rounding, and the bar the GPU result is held to.  A batch axis runs B independent
models at once (y, h ``[B, n]``); X is shared."""
import numpy as np


def _delta(sg, sh, w, lam, alpha):
    """CoordinateDelta in double, element-wise over the batch."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = w - (sg + lam * w) / (sh + lam)
        pos = np.maximum(-(sg + lam * w + alpha) / (sh + lam), -w)
        neg = np.minimum(-(sg + lam * w - alpha) / (sh + lam), -w)
    return np.where(sh < 1e-5, 0.0, np.where(t >= 0, pos, neg))


def predict_ref(X, w, b, base, ft):
    """Rule 1: p = (b + base) + x_0 w_0 + x_1 w_1 + ... in column order; X [n, F], w [B, F]."""
    p = np.repeat((b.astype(ft) + ft(base))[:, None], X.shape[0], axis=1)
    for j in range(X.shape[1]):
        p = p + X[None, :, j] * w[:, j:j + 1]
    return p


def rmse_ref(p, y, h, ft):
    d = y - p
    sq = d * d
    return np.sqrt((sq * h).astype(np.float64).sum(1) / h.astype(np.float64).sum(1))


def train_ref(X, y, h=None, *, eta=0.01, lam=100.0, alpha=0.0, lam_bias=0.0, base=2.0, rounds=100, f32=True,
              evals=()):
    """Returns (w [B, F], b [B], history [B, rounds, 1 + len(evals)]) in float64 arrays holding the
    float32 values (R32) or the float64 ones (R64).  evals: (X_e, y_e [B, n_e], h_e or None)."""
    ft = np.float32 if f32 else np.float64
    X = np.asarray(X, np.float32).astype(ft)
    y = np.atleast_2d(np.asarray(y, np.float32)).astype(ft)
    B, n = y.shape
    F = X.shape[1]
    h = np.ones((B, n), ft) if h is None else np.broadcast_to(np.atleast_2d(np.asarray(h, np.float32)), (B, n)).astype(ft)
    evals = [(np.asarray(Xe, np.float32).astype(ft), np.atleast_2d(np.asarray(ye, np.float32)).astype(ft),
              np.ones((B, np.shape(Xe)[0]), ft) if he is None else
              np.broadcast_to(np.atleast_2d(np.asarray(he, np.float32)), (B, np.shape(Xe)[0])).astype(ft))
             for Xe, ye, he in evals]
    w = np.zeros((B, F), ft)
    b = np.zeros(B, ft)
    hist = np.zeros((B, rounds, 1 + len(evals)))
    shh = h.astype(np.float64).sum(1)
    for r in range(rounds):
        p = predict_ref(X, w, b, base, ft)
        g = (p - y) * h
        sg = g.astype(np.float64).sum(1)
        db = (eta * (-(sg + lam_bias * b.astype(np.float64)) / (shh + lam_bias))).astype(ft)
        b = b + db
        g = g + h * db[:, None]
        for j in range(F):
            x = X[None, :, j]
            hx = h * x
            sgj = (g * x).astype(np.float64).sum(1)
            shj = (hx * x).astype(np.float64).sum(1)
            dw = (eta * _delta(sgj, shj, w[:, j].astype(np.float64), lam, alpha)).astype(ft)
            w[:, j] = w[:, j] + dw
            g = g + hx * dw[:, None]
        hist[:, r, 0] = rmse_ref(predict_ref(X, w, b, base, ft), y, h, ft)
        for k, (Xe, ye, he) in enumerate(evals):
            hist[:, r, 1 + k] = rmse_ref(predict_ref(Xe, w, b, base, ft), ye, he, ft)
    return w.astype(np.float64), b.astype(np.float64), hist


def noise_of(X, y, h=None, **kw):
    """(R32 [B, F+1] with the bias last, noise = max|R32 - R64| per model [B], R32 history)."""
    w32, b32, h32 = train_ref(X, y, h, f32=True, **kw)
    w64, b64, _ = train_ref(X, y, h, f32=False, **kw)
    r32 = np.concatenate([w32, b32[:, None]], 1)
    r64 = np.concatenate([w64, b64[:, None]], 1)
    return r32, np.abs(r32 - r64).max(1), h32


def make_problem(n, F, seed, B=1):
    """X [n, F] float32 with columns scaled by factors in 0.01-3, y [B, n] float32 from a sparse
    linear model plus noise, h [B, n] random integers 0-3 (float32)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, F)) * rng.uniform(0.01, 3.0, F)).astype(np.float32)
    wt = rng.standard_normal((B, F)) * (rng.random((B, F)) < 0.3)
    y = (X.astype(np.float64) @ wt.T).T + 2.0 + 0.5 * rng.standard_normal((B, n))
    h = rng.integers(0, 4, (B, n)).astype(np.float32)
    return X, y.astype(np.float32), h
