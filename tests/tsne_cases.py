"""The inputs that tests/test_gpu_tsne.py runs on the device, with their restated results computed once
(tests/tsne_ref.py).  tests/test_tsne_host.py checks on the CPU that every one of them keeps the
bisection's 1e-9 margin, so the seeds below are part of the tests' contract: change one and run that test."""
import functools

import numpy as np

import tsne_ref

NS = (2, 3, 63, 64, 65, 128, 129, 130)
DS = (1, 20)


def perplexity_of(n):
    return 1.5 if n <= 3 else 10.0 if n < 128 else 30.0


@functools.lru_cache(maxsize=None)
def affinity_cases():
    """key -> (X, perplexity).  "lat": lattice points (at d = 1 many coincide).  "dup": five copies of one
    point under perplexity 3, whose rows never meet the tolerance and run all 100 steps.  "far":
    lattice points scaled by 40, whose first steps find S == 0."""
    out = {}
    for n in NS:
        for d in DS:
            key = ("lat", n, d)
            out[key] = (tsne_ref.lattice(n, d, n + d, spread=6 if d == 1 else 4), perplexity_of(n))
    X = tsne_ref.lattice(65, 20, 7)
    X[[3, 17, 18, 40, 64]] = X[3]
    out[("dup", 65, 20)] = (X, 3.0)
    out[("far", 64, 1)] = (40.0 * np.arange(64.0)[np.random.RandomState(5).permutation(64)].reshape(64, 1), 10.0)
    for X, _ in out.values():
        X.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(key):
    """(P, beta, steps, margin) of an affinity case."""
    out = tsne_ref.affinities(*affinity_cases()[key])
    for a in out[:3]:
        a.setflags(write=False)
    return out


FULL_N, FULL_D, FULL_PERPLEXITY = 2002, 20, 30.0
FULL_ROWS = np.r_[0:8, 63:66, 997:1003, 1994:2002]


@functools.lru_cache(maxsize=None)
def full_scale():
    X = tsne_ref.lattice(FULL_N, FULL_D, 11, spread=5, centres=30)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def full_scale_reference():
    """(C rows, beta, steps, margin) of FULL_ROWS: the rows' searches do not depend on one another."""
    return tsne_ref.conditionals(full_scale(), FULL_PERPLEXITY, rows=FULL_ROWS)
