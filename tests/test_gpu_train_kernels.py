"""Edge tests of the gblinear training kernels of train.hip, called through the C entry points
(expecto_gblinear_train_round / _predict_cols / _rmse) and held bit for bit to
oracle/gblinear_train_np.py, the numpy restatement with the device's sum order.

Every comparison is equality of bits (``assert_bits``: NaN matches NaN, -0.0 differs from +0.0):
products and sums are float32 with contraction off, the row sums are a stated tree in float64,
division and sqrt in double are correctly rounded and the casts round to nearest, so nothing
here needs a tolerance.

Outputs (w, sh, pred, out) sit in ``Guarded`` buffers whose surroundings must keep their pattern.
Inputs sit in ``Margined`` allocations: at least 24,576 floats of NaN before the first column
of X (or the first model's y / h) and after the last, and NaN in rows n..ld-1 of every column.
A load that the buffer range check should have dropped, or an index off by one, reads memory
the test owns and poisons a sum; it cannot fault.

A training case runs three rounds (first = 1, then 0, 0) and compares w, sh and pred after every
round; pred is NULL in round 1."""
import numpy as np
import pytest

from gblinear_ref import make_problem
from guarded import ST, Guarded, Margined, assert_bits

from oracle import gblinear_train_np as tree

pytestmark = pytest.mark.gpu

CAP = 24576
MARGIN = CAP
HP = dict(eta=0.5, lam=1.0, alpha=0.0, lam_bias=0.0, base=2.0)


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


def last_error(lib):
    return lib.expecto_last_error().decode()


def _problem(n, F, seed, B):
    """make_problem with every model given a positive weight sum (h is integers 0..3)."""
    X, y, h = make_problem(n, F, seed=seed, B=B)
    h[h.sum(1) == 0, 0] = 1.0
    assert (h == 0).any() or n < 4
    return X, y, h


def _matrix(X, ld, shift=0):
    """The column-major device matrix of X [n, F]; None (a null X) for F = 0."""
    return Margined(X.T, ld, MARGIN, shift) if X.shape[1] else None


def _batch(a, B, stride):
    """Labels or row weights [B, n] (stride >= n), one shared row (stride 0), or None."""
    if a is None:
        return None
    a = np.atleast_2d(a)
    assert a.shape[0] == (1 if stride == 0 else B)
    return Margined(a, stride, MARGIN)


def _ptr(m):
    return None if m is None else m.ptr


def _rows(a, B):
    """The [B, n] array a Margined batch input stands for."""
    return None if a is None else np.broadcast_to(np.atleast_2d(a), (B, np.atleast_2d(a).shape[1]))


def run_rounds(lib, X, y, h, B, *, ld=None, y_stride=None, h_stride=None, shift=0, rounds=3, alone=False,
               what="", **hp):
    """Three rounds on the device against the oracle; returns the oracle's last (w, sh, pred).
    ``alone``: the oracle trains every model of the batch on its own."""
    hp = {**HP, **hp}
    n, F = X.shape
    ld = n if ld is None else ld
    y_stride = n if y_stride is None else y_stride
    h_stride = (n if h is not None else 0) if h_stride is None else h_stride
    Xd, yd, hd = _matrix(X, ld, shift), _batch(y, B, y_stride), _batch(h, B, h_stride)
    if Xd is not None and shift:
        assert Xd.ptr % 16 == 4 * shift % 16 != 0
    yy, hh = _rows(y, B), _rows(h, B)
    wd = Guarded((B, F + 1), np.float32).put(np.zeros((B, F + 1), np.float32))
    shd = Guarded((B, F), np.float64) if F else None
    w, sh = np.zeros((B, F + 1), np.float32), None
    for r in range(rounds):
        predd = Guarded((B, n), np.float32) if r else None
        st = lib.expecto_gblinear_train_round(
            _ptr(Xd), ld, n, F, B, yd.ptr, y_stride, _ptr(hd), h_stride, wd.ptr, _ptr(shd), int(r == 0), hp["eta"],
            hp["lam"], hp["alpha"], hp["lam_bias"], hp["base"], _ptr(predd), ST())
        assert st == 0, last_error(lib)
        args = (r == 0, hp["eta"], hp["lam"], hp["alpha"], hp["lam_bias"], hp["base"])
        if alone:
            parts = [tree.train_round(X, yy[m], None if hh is None else hh[m], w[m], None if r == 0 else sh[m], *args)
                     for m in range(B)]
            w, sh, pred = (np.concatenate([p[i] for p in parts]) for i in range(3))
        else:
            w, sh, pred = tree.train_round(X, yy, hh, w, sh, *args)
        tag = f"{what} n {n} F {F} B {B} ld {ld} round {r}"
        if F:
            assert_bits(shd.result(), sh, f"sh, {tag}")
        if r:
            assert_bits(predd.result(), pred, f"pred, {tag}")
        assert_bits(wd.result(), w, f"w, {tag}")
    return w, sh, pred


# ---- expecto_gblinear_train_round ----------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5000, 23553, 24575, CAP])
def test_train_round_row_edges(lib, n):
    """A lane owns rows k * 1024 + lane, k < 24, and keeps its row weights as float4 quads of four
    slots.  1 / 63 / 64 / 65: a wave's edge; 1023 / 1024 / 1025: slot 0 full, slot 1 holds one row;
    4095 / 4096 / 4097: the first quad's edge; 5000: a quad partly filled; 23553: one row in the
    last slot; 24575 / 24576: the cap."""
    X, y, h = _problem(n, 5, seed=100 + n, B=2)
    w, _, _ = run_rounds(lib, X, y, h, 2, what="row edges")
    assert np.isfinite(w).all() and (w[:, -1] != 0).all()


@pytest.mark.parametrize("n", [1003, 1025, 5000])
@pytest.mark.parametrize("pad", [0, 1, 37])
def test_train_round_poisoned_padding(lib, n, pad):
    """ld = n (row n of column j is row 0 of column j + 1), n + 1 and n + 37 with NaN in the
    padding, the matrix 4 bytes off a 16-byte boundary: the range check of the column's buffer
    descriptor, and nothing the padding holds, keeps rows past n out of the sums.  The oracle
    sees the unpadded matrix."""
    X, y, h = _problem(n, 5, seed=200 + n, B=2)
    w, _, _ = run_rounds(lib, X, y, h, 2, ld=n + pad, shift=1, what="poisoned padding")
    assert np.isfinite(w).all()


@pytest.mark.parametrize("F", [0, 1, 2, 3, 4])
def test_train_round_feature_edges(lib, F):
    """The column loops handle two columns a trip through two register buffers: F = 1 / 3 leave
    the loop in the middle of a trip, 2 / 4 at its end.  F = 0 is called with null X and sh, and
    only the bias moves."""
    X, y, h = _problem(1025, F, seed=300 + F, B=2)
    w, _, _ = run_rounds(lib, X, y, h, 2, what="F edges")
    assert w.shape == (2, F + 1) and (w[:, F] != 0).all()


@pytest.mark.parametrize("mode", ["shared y, h stride n + 5", "y stride n + 3, no h", "both shared"])
def test_train_round_strides(lib, mode):
    n, B = 1025, 3
    X, y, h = _problem(n, 4, seed=400, B=B)
    if mode == "shared y, h stride n + 5":
        kw = dict(y=y[:1], h=h, y_stride=0, h_stride=n + 5)
    elif mode == "y stride n + 3, no h":
        kw = dict(y=y, h=None, y_stride=n + 3, h_stride=0)
    else:
        kw = dict(y=y[:1], h=h[:1], y_stride=0, h_stride=0)
    w, _, _ = run_rounds(lib, X, kw.pop("y"), kw.pop("h"), B, alone=True, what=mode, **kw)
    same = [np.array_equal(w[0], w[m]) for m in (1, 2)]
    assert all(same) if mode == "both shared" else not any(same)


def test_train_round_more_workgroups_than_cus(lib):
    X, y, h = _problem(65, 3, seed=500, B=257)
    w, _, _ = run_rounds(lib, X, y, h, 257, what="257 models")
    assert len({w[m].tobytes() for m in range(257)}) == 257


@pytest.mark.parametrize("base", [0.0, -1.25])
@pytest.mark.parametrize("lam_bias", [0.5, 100.0])
def test_train_round_bias_terms(lib, lam_bias, base):
    X, y, h = _problem(1025, 3, seed=600, B=2)
    w0, _, _ = run_rounds(lib, X, y, h, 2, what="lambda_bias 0")
    w1, _, _ = run_rounds(lib, X, y, h, 2, lam_bias=lam_bias, base=base, what=f"lambda_bias {lam_bias} base {base}")
    assert (w0[:, -1] != w1[:, -1]).all()


def test_train_round_l1_leaves_exact_zeros(lib):
    """alpha = 50 clips some weights to exactly zero (-w is the step: w + (-w) = +0.0) and moves
    others; the zero's sign bit is compared like every other bit."""
    X, y, h = _problem(1025, 12, seed=11, B=2)
    w, _, _ = run_rounds(lib, X, y, h, 2, alpha=50.0, what="alpha 50")
    zero = w[:, :-1] == 0
    assert zero.any() and (~zero).any() and not np.signbit(w[:, :-1][zero]).any()


def test_train_round_full_step_without_ridge(lib):
    X, y, h = _problem(1025, 4, seed=700, B=2)
    run_rounds(lib, X, y, h, 2, eta=1.0, lam=0.0, what="eta 1 lambda 0")


def test_train_round_flat_columns(lib):
    """A column of zeros and one of 1e-4 under 0 / 1 row weights: sh < 1e-5, so the weight stays
    at 0, and sh (0 and about 1e-8 * sum h) is still stored."""
    X, y, h = _problem(1025, 5, seed=800, B=2)
    X[:, 1], X[:, 3] = 0.0, 1e-4
    h = np.minimum(h, 1.0)
    w, sh, _ = run_rounds(lib, X, y, h, 2, what="flat columns")
    assert (sh[:, 1] == 0).all() and (sh[:, 3] > 0).all() and (sh[:, 3] < 1e-5).all()
    assert (w[:, [1, 3]] == 0).all() and (w[:, [0, 2, 4]] != 0).all()


def test_train_round_isolation(lib):
    """The middle model of three has all row weights 0: its bias step is 0 / 0 and its bias and
    predictions are NaN from then on, in the oracle and on the device.  Its neighbours keep the
    bits they have when trained alone."""
    X, y, h = _problem(1025, 4, seed=900, B=3)
    h[1] = 0.0
    w, _, pred = run_rounds(lib, X, y, h, 3, alone=True, what="isolation")
    assert np.isnan(w[1, -1]) and np.isnan(pred[1]).all()
    assert np.isfinite(w[[0, 2]]).all() and np.isfinite(pred[[0, 2]]).all()


# ---- expecto_gblinear_predict_cols ---------------------------------------------------------

F32_TINY = np.finfo(np.float32).tiny
# values whose products with each other round, vanish into or come out of the float32 subnormals
SPECIAL = np.array([1 + 2.0 ** -23, 1 - 2.0 ** -24, 2.0 ** -140, 1e-39, -3e-41, -0.0, 0.0, 3.0000002, -(1 + 2.0 ** -22),
                    2.0 ** -75, -(2.0 ** -74) * 1.25, 2.0 ** 100, F32_TINY, -F32_TINY * 0.75], np.float32)


def _predict_cols(lib, Xd, ld, n, F, B, w, base):
    out = Guarded((B, n), np.float32)
    wd = Margined(w, F + 1, 64)
    st = lib.expecto_gblinear_predict_cols(_ptr(Xd), ld, n, F, B, wd.ptr, base, out.ptr, ST())
    assert st == 0, last_error(lib)
    return out.result()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_predict_cols_edges(lib, n):
    """Rows around the 256-row workgroup, columns 0 / 1 / 7 / 8 / 9 / 17 around the 8-column chunk,
    three models, ld > n with NaN padding.  Planted: subnormal values and weights, products that
    are subnormal (2^-75 * 2^-74 * 1.25), that underflow to zero and that round."""
    rng = np.random.default_rng(1000 + n)
    B, ld = 3, n + 11
    for F in (0, 1, 7, 8, 9, 17):
        X = rng.standard_normal((n, F)).astype(np.float32)
        w = rng.standard_normal((B, F + 1)).astype(np.float32)
        if F:
            X[rng.integers(0, n, 40), rng.integers(0, F, 40)] = SPECIAL[rng.integers(0, SPECIAL.size, 40)]
            X[0, :] = np.resize(SPECIAL, F)
            w[0, :F] = np.resize(SPECIAL[::-1], F)
            w[1, :F] = np.resize(np.roll(SPECIAL, 5), F)
        if F == 1:
            w[2, 1], X[0, 0], w[2, 0] = 0.0, 2.0 ** -75, -(2.0 ** -74) * 1.25       # a lone subnormal product
        base = (0.5, -1.25)[F % 2] if F != 1 else 0.0
        want = tree.predict_cols(X, w, base)
        got = _predict_cols(lib, _matrix(X, ld), ld, n, F, B, w, base)
        assert_bits(got, want, f"predict_cols n {n} F {F}")
        if F == 1:
            assert want[2, 0] != 0 and abs(want[2, 0]) < F32_TINY
        if F == 0:
            assert_bits(got, np.repeat((w[:, 0] + np.float32(base))[:, None], n, 1), "bias and base alone")


def test_round_pred_is_predict_cols_of_the_round_before(lib):
    """The kernels against each other: the pred a training round writes equals
    expecto_gblinear_predict_cols of the weights the round before left, bit for bit."""
    n, F, B, ld = 1025, 5, 2, 1030
    X, y, h = _problem(n, F, seed=1100, B=B)
    Xd, yd, hd = _matrix(X, ld), _batch(y, B, n), _batch(h, B, n)
    wd = Guarded((B, F + 1), np.float32).put(np.zeros((B, F + 1), np.float32))
    shd = Guarded((B, F), np.float64)
    for r in range(3):
        before = wd.result()
        predd = Guarded((B, n), np.float32)
        st = lib.expecto_gblinear_train_round(Xd.ptr, ld, n, F, B, yd.ptr, n, hd.ptr, n, wd.ptr, shd.ptr, int(r == 0),
                                              0.5, 1.0, 0.0, 0.0, 2.0, predd.ptr, ST())
        assert st == 0, last_error(lib)
        assert_bits(predd.result(), _predict_cols(lib, Xd, ld, n, F, B, before, 2.0), f"pred of round {r}")
    assert (wd.result() != before).all()


# ---- expecto_gblinear_rmse -----------------------------------------------------------------

@pytest.mark.parametrize("hmode", ["no h", "shared h", "h stride n + 5"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000])
def test_rmse_edges(lib, n, hmode):
    """Lane t adds rows t, t + 1024, ...: one partly filled pass, exactly one, one row into the
    second, and five passes.  The residuals' squares round in float32, and so do their products
    with the weights 0..3."""
    B = 3
    rng = np.random.default_rng(1200 + n)
    pred = rng.standard_normal((B, n)).astype(np.float32) * 3
    y = rng.standard_normal((B, n)).astype(np.float32)
    h = rng.integers(0, 4, (B, n)).astype(np.float32)
    h[:, 0] = 3.0
    if hmode == "no h":
        h, y_stride, h_stride = None, n + 3, 0
    elif hmode == "shared h":
        h, y, y_stride, h_stride = h[:1], y[:1], 0, 0
    else:
        y_stride, h_stride = n, n + 5
    d = (_rows(y, B) - pred).astype(np.float64)
    assert (np.float32(d * d).astype(np.float64) != d * d).any()
    predd, yd, hd = Margined(pred, n, MARGIN), _batch(y, B, y_stride), _batch(h, B, h_stride)
    out = Guarded((B,), np.float64)
    st = lib.expecto_gblinear_rmse(predd.ptr, yd.ptr, y_stride, _ptr(hd), h_stride, n, B, out.ptr, ST())
    assert st == 0, last_error(lib)
    want = tree.rmse(pred, _rows(y, B), _rows(h, B))
    assert np.isfinite(want).all() and (want > 0).all()
    assert_bits(out.result(), want, f"rmse n {n}, {hmode}")


# ---- refusals ------------------------------------------------------------------------------

def test_refusals_write_nothing(lib):
    n, F, B = 70, 3, 2
    X, y, h = _problem(n, F, seed=1300, B=B)
    Xd, yd, hd = _matrix(X, n), _batch(y, B, n), _batch(h, B, n)
    w0 = np.zeros((B, F + 1), np.float32)
    wd, pd = Margined(w0, F + 1, 64), Margined(np.zeros((B, n), np.float32), n, 64)
    wout, sh, pred = Guarded((B, F + 1), np.float32), Guarded((B, F), np.float64), Guarded((B, n), np.float32)
    out, rm = Guarded((B, n), np.float32), Guarded((B,), np.float64)

    def train(ld=n, n=n, F=F, B=B, w=wout.ptr):
        return lib.expecto_gblinear_train_round(Xd.ptr, ld, n, F, B, yd.ptr, n, hd.ptr, n, w, sh.ptr, 1, 0.5, 1.0, 0.0,
                                                0.0, 2.0, pred.ptr, ST())

    def predict(ld=n, n=n, F=F, B=B, w=wd.ptr):
        return lib.expecto_gblinear_predict_cols(Xd.ptr, ld, n, F, B, w, 2.0, out.ptr, ST())

    def rmse(n=n, B=B, p=pd.ptr):
        return lib.expecto_gblinear_rmse(p, yd.ptr, n, hd.ptr, n, n, B, rm.ptr, ST())

    for call in (train, predict):
        assert call(ld=n - 1) == -1 and "ld >= n" in last_error(lib)
        for neg in (dict(n=-1), dict(F=-1), dict(B=-1)):
            assert call(**neg) == -1 and "negative shape" in last_error(lib), neg
        assert call(w=None) == -1 and "null" in last_error(lib)
        assert call(n=0) == 0 and call(B=0) == 0
    assert predict(B=65536) == -1 and "65535" in last_error(lib)
    assert rmse(n=-1) == -1 and rmse(B=-1) == -1 and "negative shape" in last_error(lib)
    assert rmse(p=None) == -1 and "null" in last_error(lib)
    assert rmse(n=0) == 0 and rmse(B=0) == 0
    for g in (wout, sh, pred, out, rm):
        assert g.untouched()
