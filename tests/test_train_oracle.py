"""CPU: anchors oracle/gblinear_train_np.py, the restatement of the training kernels with the
device's sum order that test_gpu_train_kernels.py holds the kernels to bit for bit.

It is the steps of gblinear_ref.train_ref (R32) with another order of the double sums, so after
the same rounds its [w; b] must lie within noise = max|R32 - R64| of R32 (the bar
test_gpu_train.py uses for the kernels), and its tree sum must be a sum."""
import math

import numpy as np
import pytest

from gblinear_ref import make_problem, noise_of

from oracle.gblinear_train_np import LANES, predict_cols, rmse, train_round, tree_sum


def _train(X, y, h, eta, lam, rounds, base=2.0):
    w = np.zeros((y.shape[0], X.shape[1] + 1), np.float32)
    sh = None
    for r in range(rounds):
        w, sh, pred = train_round(X, y, h, w, sh, r == 0, eta, lam, 0.0, 0.0, base)
    return w, sh, pred


@pytest.mark.parametrize("n,F,eta,lam,rounds", [(1003, 97, 0.01, 100.0, 5), (1003, 97, 0.5, 1.0, 8),
                                                (1003, 97, 1.0, 0.0, 3), (5000, 7, 0.5, 1.0, 4),
                                                (24575, 3, 0.5, 1.0, 4)])
def test_tree_oracle_within_noise_of_r32(n, F, eta, lam, rounds):
    X, y, h = make_problem(n, F, seed=11)
    r32, noise, hist = noise_of(X, y, h, eta=eta, lam=lam, rounds=rounds)
    w, sh, pred = _train(X, y, h, eta, lam, rounds)
    err = np.abs(w.astype(np.float64) - r32).max(1)
    same = (w == r32.astype(np.float32)).mean()
    numpy_sh = ((h[0] * X.T) * X.T).astype(np.float64).sum(1)
    print(f"n={n} F={F} eta={eta} lambda={lam}: max|tree - R32| {err.max():.3g}, noise {noise.min():.3g}, "
          f"bit-equal share {same:.4f}, sh equal to numpy's sum in {(sh[0] == numpy_sh).mean():.2f} of the columns")
    assert (err <= noise).all(), (err, noise)
    np.testing.assert_allclose(sh[0], numpy_sh, rtol=n * 2.0 ** -53)
    # rule 6 on the last round's weights; pred is one round behind, so evaluate afresh
    np.testing.assert_allclose(rmse(predict_cols(X, w, 2.0), y, h), hist[:, -1, 0], rtol=1e-5)


@pytest.mark.parametrize("n", [1, 1025, 24576])
def test_tree_sum_is_a_sum(n):
    """Any order of n - 1 double additions errs by at most (n - 1) * 2^-53 * sum|v| (to first order;
    n * 2^-53 covers the rest)."""
    rng = np.random.default_rng(n)
    v = rng.standard_normal((3, n)) * 10.0 ** rng.integers(-3, 4, (3, n))
    got = tree_sum(v)
    for b in range(3):
        assert abs(got[b] - math.fsum(v[b])) <= n * 2.0 ** -53 * math.fsum(np.abs(v[b]))
    assert tree_sum(v[0]).shape == () and tree_sum(v[0]) == got[0]


def test_tree_sum_order():
    """The order itself, on terms where it shows: 2^53 + 1 + 1 is 2^53 if the ones arrive one at a
    time and 2^53 + 2 if they arrive as a pair."""
    big = 2.0 ** 53
    v = np.zeros(2 * LANES)
    v[0], v[1], v[LANES] = big, 1.0, 1.0            # lane 0: (big + 1) = big; + lane 1's 1 -> big
    assert tree_sum(v) == big
    v = np.zeros(2 * LANES)
    v[0], v[2], v[3] = big, 1.0, 1.0                # lanes 2 and 3 pair first: big + 2
    assert tree_sum(v) == big + 2.0
    v = np.zeros(2 * LANES)
    v[0], v[1], v[2] = big, 1.0, 1.0                # (big + 1) + (1 + 0) = big + 1 -> ties to even
    assert tree_sum(v) == big
    assert math.copysign(1.0, tree_sum(np.array([-0.0]))) == 1.0       # every lane starts at +0.0
