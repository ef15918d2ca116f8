"""numpy restatement of the saturation-mutagenesis entry points (expecto_ism_variants,
expecto_ism_score, expecto_ism_summary; include/expecto_hip.h) -- TEST INFRASTRUCTURE ONLY.

The score is the unfused chain written out: float32 fwd/rc average, float64 exp-decay reduction and
float32 serial gblinear scoring, each taken from the oracle (oracle/reduce_np.py,
oracle/gblinear_np.py), not re-derived."""
import numpy as np

from oracle import gblinear_np, reduce_np


def variants(codes, start, L):
    """(var_off int64, ref_code, alt_code, valid uint8), 3 L slots, slot 3*p + j."""
    ref = np.asarray(codes, np.uint8)[start:start + L]
    base = ref < 4
    j = np.arange(3, dtype=np.uint8)[None, :]
    alt = np.where(base[:, None], j + (j >= ref[:, None]), ref[:, None]).astype(np.uint8)
    return (np.repeat(np.arange(start, start + L, dtype=np.int64), 3), np.repeat(ref, 3), alt.reshape(-1),
            np.repeat(base.astype(np.uint8), 3))


def features(y, dist, strand_plus, shifts):
    """y [2 strands, S, n, F] float32 -> float64 [n, 10 F]: the average, then the reduction."""
    _, S, n, F = y.shape
    avg = reduce_np.fwd_rc_average(np.ascontiguousarray(y, np.float32).reshape(2 * S * n, F)).reshape(S, n, F)
    w = reduce_np.variant_weights(dist, np.full(n, bool(strand_plus)), shifts)
    return reduce_np.variant_reduce(list(avg), w, F)


def chain(y, dist, strand_plus, shifts, keep, w, init):
    """float32 [M, n]: model m's predictions of the rows of one allele; w [10 nk, M], init [M]."""
    F = y.shape[3]
    mask = np.zeros(F, bool)
    mask[np.asarray(keep)] = True
    x = features(y, dist, strand_plus, shifts)[:, gblinear_np.keep_columns(mask, F)]
    return np.stack([gblinear_np.predict(x, w[:, m], init[m], 0.0) for m in range(w.shape[1])])


def score(y_ref, y_alt, dist, strand_plus, shifts, keep, w, init, valid):
    """(alt_pred f32 [M, n], ref_pred f32 [M, n/3], sed f64 [M, n])."""
    valid = np.asarray(valid, bool)
    ref = chain(y_ref, dist, strand_plus, shifts, keep, w, init)[:, 0::3]
    alt = chain(y_alt, dist, strand_plus, shifts, keep, w, init)
    sed = alt.astype(np.float64) - np.repeat(ref, 3, axis=1).astype(np.float64)
    alt[:, ~valid] = np.nan
    sed[:, ~valid] = np.nan
    ref[:, ~valid.reshape(-1, 3).any(1)] = np.nan
    return alt, ref, sed


def S(x):
    """The fixed summation order of expecto_variant_contrib (include/expecto_hip.h)."""
    x = np.asarray(x, np.float64).reshape(-1)
    if x.size == 0:
        return np.float64(0.0)
    p = np.full(64, -0.0)
    for i in range(x.size):
        p[i % 64] = p[i % 64] + x[i]
    s = 32
    while s:
        p[:s] = p[:s] + p[s:2 * s]
        s >>= 1
    return p[0]


def summaries(sed, valid):
    """(variation_potential, directionality) float64 [M]: an invalid slot's term is -0.0."""
    valid = np.asarray(valid, bool)
    vp = np.array([S(np.where(valid, np.abs(r), -0.0)) for r in sed])
    dr = np.array([S(np.where(valid, r, -0.0)) for r in sed])
    return vp, dr
