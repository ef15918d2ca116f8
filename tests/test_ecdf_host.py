"""CPU: the two-level lower bound of expecto_ecdf_tail_counts (expecto_amd/csrc/ecdf_search.h) built
with the host compiler alone into tests/ecdf_search_driver.cpp, as test_ward_host.py builds the
linkage, and compared with ``np.searchsorted`` (tests/ecdf_ref.py) -- once more under the address
and undefined-behaviour sanitizers, run directly."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ecdf_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "ecdf_search_driver.cpp")
K = int(re.search(r"#define EXPECTO_ECDF_SPLITTERS (\d+)", open(os.path.join(REPO, "include", "expecto_hip.h")).read())
        .group(1))


def lengths(k):
    return [1, 2, 3, k - 1, k, k + 1, 2 * k - 1, 2 * k + 1, 5 * k + 7]


def plan(B, k):
    stride = -(-B // k)
    return stride, -(-B // stride)


def probes(col, k):
    """Queries below, at and above every splitter, the ends, +-0, a denormal, +-inf and NaN."""
    stride, m = plan(col.size, k)
    s = col[np.arange(m) * stride]
    with np.errstate(all="ignore"):
        q = np.concatenate([s, np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf)), col[-1:],
                            np.nextafter(col[-1:], np.float32(np.inf)),
                            np.array([0.0, -0.0, 1e-41, np.inf, -np.inf, np.nan, 0.5], np.float32)])
    return q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, K, column, queries)]: every length of the list at the kernel's K and at K = 8, random
    columns with ties, columns of one value, and runs of ties laid across splitters."""
    out = []
    rng = np.random.default_rng(11)
    for k in (K, 8):
        for B in lengths(k):
            if B < 1:
                continue
            col = ecdf_ref.background(1, B, seed=B)[0]
            out.append((f"K{k}-B{B}-random", k, col))
            out.append((f"K{k}-B{B}-equal", k, np.full(B, 0.25, np.float32)))
            stride, m = plan(B, k)
            ties = np.sort(rng.random(B).astype(np.float32))
            for i in range(1, m, max(1, m // 5)):      # a run of equal values around splitter i
                lo, hi = max(0, i * stride - stride // 2 - 1), min(B, i * stride + stride // 2 + 2)
                ties[lo:hi] = ties[lo]
            assert (np.diff(ties) >= 0).all()
            out.append((f"K{k}-B{B}-straddle", k, ties))
    full = []
    for name, k, col in out:
        col.setflags(write=False)
        full.append((name, 0 if k == K else k, col, probes(col, k)))
    return full


@functools.lru_cache(maxsize=None)
def expected():
    """The search takes the query as it is (the kernel hands it |x|): a negative one counts everything."""
    out = []
    for _, _, col, q in cases():
        want = (col.size - np.searchsorted(col, q, side="left")).astype(np.int32)
        want[np.isnan(q)] = -1
        assert np.array_equal(want[q >= 0], ecdf_ref.tail_counts(col[None], q[q >= 0][:, None], [0])[:, 0])
        out.append(want)
    return out


def _cxx():
    return [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]


def _word(v):
    v = float(v)
    return v.hex() if np.isfinite(v) else repr(v)


def run_driver(exe):
    text = "".join(f"{k} {col.size} {q.size}\n" + " ".join(map(_word, col)) + "\n" + " ".join(map(_word, q)) + "\n"
                   for _, k, col, q in cases())
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    plans, counts = [], []
    for ln in res.stdout.splitlines():
        word, _, rest = ln.partition(" ")
        if word == "case":
            counts.append([])
        elif word == "plan":
            plans.append(tuple(map(int, rest.split())))
        elif word == "ge":
            counts[-1].append(tuple(map(int, rest.split())))
    return plans, [np.array(c, np.int32).reshape(-1, 2) for c in counts], res.stdout


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ecdf") / "ecdf_search_driver")
    subprocess.run(_cxx() + ["-std=c++17", "-O2", "-Wall", SRC, "-o", exe], check=True)
    return run_driver(exe)


def test_plans(driver_output):
    plans = driver_output[0]
    assert len(plans) == len(cases())
    for (name, k, col, _), (stride, m, pick, finish) in zip(cases(), plans):
        k = k or K
        assert (stride, m) == plan(col.size, k), name
        assert 1 <= m <= k and (m - 1) * stride < col.size <= m * stride, name
        assert pick == int(m).bit_length() and finish == int(stride - 1).bit_length(), name
        if col.size <= k:
            assert stride == 1 and m == col.size and finish == 0, name


def test_counts_equal_searchsorted(driver_output):
    _, counts, _ = driver_output
    for (name, _, _, q), got, want in zip(cases(), counts, expected()):
        assert got.shape == (q.size, 2), name
        assert np.array_equal(got[:, 0], want), (name, "one query at a time")
        assert np.array_equal(got[:, 1], want), (name, "four queries side by side")


def test_cases_cover_the_edges():
    names = [c[0] for c in cases()]
    for B in lengths(K):
        assert f"K{K}-B{B}-straddle" in names
    _, _, col, q = cases()[names.index(f"K{K}-B{5 * K + 7}-straddle")]
    stride, m = plan(col.size, K)
    assert stride == 6 and (col[stride * 1 - 1] == col[stride * 1] == col[stride * 1 + 1])   # a run across a splitter
    assert np.isnan(q).any() and np.isinf(q).any() and (q == col[0]).any()
    want = expected()[names.index(f"K{K}-B{5 * K + 7}-equal")]
    assert set(want.tolist()) == {-1, 0, 5 * K + 7}                                           # all ties: all or nothing


def test_driver_under_sanitizers(tmp_path, driver_output):
    """The same driver built with -fsanitize=address,undefined and run directly: the same output, no
    report.  The driver sizes the column and the splitter array exactly, so a read past either is
    reported."""
    exe = str(tmp_path / "ecdf_search_driver_san")
    build = subprocess.run(_cxx() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                                     "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the host compiler has no address/undefined sanitizer runtime: " + build.stderr[-200:])
    assert run_driver(exe)[2] == driver_output[2]
