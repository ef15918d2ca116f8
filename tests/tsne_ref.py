"""numpy restatement of the t-SNE contract of include/expecto_hip.h (expecto_tsne_affinities,
expecto_tsne_descend) and of the staged driver of ``cluster_and_viz.tsne``: the bits the device must
give, up to the ulps of ``exp`` and ``log``.  Every product and sum is a separate float64 numpy
operation, so nothing is fused; every sum is :func:`wave_sum`.  Also the fixed inputs of the sklearn
fixture (tests/golden/make_golden_tsne.py) and of the device tests."""
import numpy as np

EPS = np.finfo(np.float64).eps
TOL = 1e-5
MAX_STEPS = 100
FLOAT_MAX = np.finfo(np.float64).max


def wave_sum(a):
    """The wave-order sum over the last axis: a [..., m] -> [...].  The terms are laid out as
    [ceil(m / 64), 64] padded with +0.0; lane l's chain is the sequential sum down column l from +0.0
    (a chain never holds -0.0, so the padding changes nothing); then the six folds."""
    a = np.asarray(a, np.float64)
    m = a.shape[-1]
    rows = -(-m // 64)
    pad = np.zeros(a.shape[:-1] + (rows * 64,))
    pad[..., :m] = a
    pad = pad.reshape(a.shape[:-1] + (rows, 64))
    s = np.zeros(a.shape[:-1] + (64,))
    for r in range(rows):
        s = s + pad[..., r, :]
    for w in (32, 16, 8, 4, 2, 1):
        s = s[..., :w] + s[..., w:2 * w]
    return s[..., 0]


def sqdist(A, B):
    """[a, b]: s = +0.0; for t ascending u = A[i, t] - B[j, t]; s = s + u*u."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    s = np.zeros((A.shape[0], B.shape[0]))
    for t in range(A.shape[1]):
        u = A[:, t, None] - B[None, :, t]
        s = s + u * u
    return s


def conditionals(X, perplexity, rows=None):
    """The bisection of the rows ``rows`` (all by default).  Returns (C [len(rows), n], beta, steps int32,
    margin): margin is the least distance, over every step of every row, of |H - log(perplexity)| from 0
    and from the tolerance -- a branch can flip under other ulps of exp and log only where it is tiny."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    D = sqdist(X[rows], X)
    m = rows.size
    logp = np.log(perplexity)
    beta, lo, hi = np.ones(m), np.full(m, -np.inf), np.full(m, np.inf)
    used, steps, C = np.ones(m), np.zeros(m, np.int32), np.zeros((m, n))
    active = np.arange(m)
    margin = np.inf
    for step in range(MAX_STEPS):
        if active.size == 0:
            break
        Da, b = D[active], beta[active]
        p = np.exp(-Da * b[:, None])
        p[np.arange(active.size), rows[active]] = 0.0
        S = wave_sum(p)
        S[S == 0.0] = 1e-8
        p = p / S[:, None]
        H = np.log(S) + b * wave_sum(Da * p)
        diff = H - logp
        margin = min(margin, np.abs(diff).min(), np.abs(np.abs(diff) - TOL).min())
        used[active], steps[active], C[active] = b, step + 1, p
        done = np.abs(diff) <= TOL
        up = ~done & (diff > 0.0)
        down = ~done & ~up
        a_up, a_dn = active[up], active[down]
        lo[a_up] = beta[a_up]
        beta[a_up] = np.where(hi[a_up] == np.inf, beta[a_up] * 2.0, (beta[a_up] + hi[a_up]) / 2.0)
        hi[a_dn] = beta[a_dn]
        beta[a_dn] = np.where(lo[a_dn] == -np.inf, beta[a_dn] / 2.0, (beta[a_dn] + lo[a_dn]) / 2.0)
        active = active[~done]
    return C, used, steps, float(margin)


def joint(C):
    V = C + C.T
    T = wave_sum(wave_sum(V))
    P = np.maximum(V / max(T, EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def affinities(X, perplexity):
    """(P [n, n], beta [n], steps int32 [n], margin)."""
    C, beta, steps, margin = conditionals(X, perplexity)
    return joint(C), beta, steps, margin


def iterate(P, exaggeration, Y, update, gains, momentum, learning_rate, want_error=True):
    """One iteration: (Y, update, gains, stats [error, grad_norm, Z], sum of the error's |terms|)."""
    a = Y[:, None, 0] - Y[None, :, 0]
    b = Y[:, None, 1] - Y[None, :, 1]
    num = 1.0 / (1.0 + (a * a + b * b))
    off = num.copy()
    np.fill_diagonal(off, 0.0)
    Z = wave_sum(wave_sum(off))
    q = np.maximum(num / Z, EPS)
    pe = exaggeration * P
    t = (pe - q) * num
    ta, tb = t * a, t * b
    np.fill_diagonal(ta, 0.0)
    np.fill_diagonal(tb, 0.0)
    g = 4.0 * np.stack([wave_sum(ta), wave_sum(tb)], axis=1)
    gains = np.where(update * g < 0.0, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, 0.01)
    g = g * gains
    update = momentum * update - learning_rate * g
    Y = Y + update
    err, mass = np.nan, 0.0
    if want_error:
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = pe * np.log(np.maximum(pe, EPS) / q)
        np.fill_diagonal(terms, 0.0)
        err, mass = wave_sum(wave_sum(terms)), float(np.abs(terms).sum())
    stats = np.array([err, np.sqrt(wave_sum((g * g).ravel())), Z])
    return Y, update, gains, stats, mass


def descend(P, exaggeration, Y, update, gains, momentum, learning_rate, n_iter, want_error=True):
    """expecto_tsne_descend: (Y, update, gains, stats, mass) after n_iter >= 1 iterations."""
    for it in range(n_iter):
        Y, update, gains, stats, mass = iterate(P, exaggeration, Y, update, gains, momentum, learning_rate,
                                                want_error and it == n_iter - 1)
    return Y, update, gains, stats, mass


def staged(P, Y0, early_exaggeration=12.0, learning_rate=50.0, max_iter=1000, exploration_iter=250, n_iter_check=50,
           n_iter_without_progress=300, min_grad_norm=1e-7, descend=descend):
    """sklearn's two calls of _gradient_descent in chunks that end at its check points and at the stages'
    ends.  Returns (Y, kl_divergence, iterations run, [(iteration, error, grad_norm)] of the check points)."""
    Y = np.array(Y0, np.float64)
    n = Y.shape[0]
    done, kl, checks = 0, np.nan, []
    first = min(exploration_iter, max_iter)
    for end, momentum, exaggeration, window in ((first, 0.5, early_exaggeration, exploration_iter),
                                                (max_iter, 0.8, 1.0, n_iter_without_progress)):
        update, gains = np.zeros((n, 2)), np.ones((n, 2))
        best, best_iter = FLOAT_MAX, done
        while done < end:
            nxt = min(end, (done // n_iter_check + 1) * n_iter_check)
            Y, update, gains, stats = descend(P, exaggeration, Y, update, gains, momentum, learning_rate, nxt - done)[:4]
            done, kl = nxt, float(stats[0])
            if done % n_iter_check == 0:
                checks.append((done, kl, float(stats[1])))
                if kl < best:
                    best, best_iter = kl, done - 1
                elif done - 1 - best_iter > window:
                    break
                if stats[1] <= min_grad_norm:
                    break
    return Y, kl, done, checks


def pca_init(X):
    """The first two principal scores of X, signs by sklearn's svd_flip on v, std of the first 1e-4."""
    X = np.asarray(X, np.float64)
    U, S, Vt = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)
    signs = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
    Y = (U * signs)[:, :2] * S[:2]
    return Y / np.std(Y[:, 0]) * 1e-4


# ---- inputs ----------------------------------------------------------------------------------

def lattice(n, d, seed, spread=4, centres=3):
    """n points with small-integer coordinates around ``centres`` integer centres: every squared distance
    is an integer below 2^24, exact in float32."""
    rng = np.random.RandomState(seed)
    c = rng.randint(-12, 13, size=(centres, d))
    X = c[rng.randint(0, centres, size=n)] + rng.randint(-spread, spread + 1, size=(n, d))
    return X.astype(np.float64)


def start(n, seed):
    return 1e-4 * np.random.RandomState(seed).standard_normal((n, 2))


# The sklearn fixture: name -> (n, d, input seed, perplexity, early_exaggeration, learning_rate, max_iter).
# sklearn's gains (+0.2 per iteration while a gradient entry keeps its sign) raise the step until the
# descent oscillates, and from there on it multiplies a rounding-size change of Y by about ten every
# twenty iterations: with the default learning rate (at least 50) two float64 implementations that differ
# in summation order alone end with unrelated pictures at these n.  The cases use rates at which the 300
# iterations that sklearn insists on stay on the smooth side, so that the comparison is of algorithms.
CASES = {
    "lattice60": (60, 5, 1, 10.0, 1.0, 1.0, 300),
    "lattice130": (130, 20, 2, 30.0, 2.0, 1.0, 300),
}


# The restatement against sklearn on these cases (tests/test_tsne_host.py states the measured values):
# 100 x the largest max |dY| / std(Y) and the largest relative difference of the KL divergence seen.
Y_BOUND = 1.4e-6
KL_BOUND = 1.3e-8


def case_inputs(name):
    """(X, Y0, keyword arguments of sklearn's TSNE and of ``staged`` alike)."""
    n, d, seed, perplexity, exaggeration, rate, max_iter = CASES[name]
    return lattice(n, d, seed), start(n, seed + 100), dict(perplexity=perplexity, early_exaggeration=exaggeration,
                                                           learning_rate=rate, max_iter=max_iter)
