"""GPU: expecto_ecdf_tail_counts and expecto_ecdf_summary through the C ABI on guarded buffers, bit
for bit against the numpy restatement (tests/ecdf_ref.py): every background length at which the
two-level search takes another path, variant counts around the 64-lane wave and the 256-variant
tile, column counts around the 16-column tile and the 64-term lanes of the order S, a sparse column
map into C = 2002 marks whose unused rows and columns hold NaN, and every refusal."""
import functools

import numpy as np
import pytest

import ecdf_ref
from guarded import Guarded, P, ST, assert_bits, dev_offset
from test_ecdf_host import K, lengths

pytestmark = pytest.mark.gpu

C = 2002
EINVAL = -1
NS = [1, 63, 64, 65, 130]
NCS = [1, 63, 64, 65, 2002]


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def column_map(nc):
    """nc ascending marks of the C: sparse and irregular, the last mark among them."""
    if nc == C:
        return np.arange(C, dtype=np.int32)
    rng = np.random.default_rng(nc)
    cols = np.sort(rng.choice(C - 1, nc - 1, replace=False)).astype(np.int32) if nc > 1 else np.empty(0, np.int32)
    return np.append(cols, C - 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(B, nc, n):
    """Host inputs and the restatement's outputs, computed once: rows [nc, B] (the background of the
    mapped marks), x [n, C + 5] with NaN in every column outside the map, one NaN query."""
    cols = column_map(nc)
    rows = ecdf_ref.background(nc, B, seed=B + nc)
    x = np.full((n, C + 5), np.nan, np.float32)
    x[:, cols] = ecdf_ref.queries(rows, n, nc, seed=B + nc + n)
    if n >= 2:
        x[n // 2, cols[nc // 2]] = np.nan
    ge = ecdf_ref.tail_counts(rows, x[:, cols], np.arange(nc))
    table = ecdf_ref.lut(B)
    sums = {k: ecdf_ref.summaries(ge, table, k) for k in (0, 1, B + 1)}
    for a in (cols, rows, x, ge, table) + tuple(v for s in sums.values() for v in s):
        a.setflags(write=False)
    return dict(B=B, nc=nc, n=n, cols=cols, rows=rows, x=x, ge=ge, table=table, sums=sums)


def device_background(c):
    """[C, B] on the device, off alignment: the mapped rows, NaN everywhere else."""
    full = np.full((C, c["B"]), np.nan, np.float32)
    full[c["cols"]] = c["rows"]
    return dev_offset(full, 8)


def run_both(lib, c):
    bg, x = device_background(c), dev_offset(c["x"], 4)
    cols_d = dev_offset(c["cols"], 4)
    n, nc, B = c["n"], c["nc"], c["B"]
    ge = Guarded((n, nc), np.int32, offset=4)
    st = lib.expecto_ecdf_tail_counts(P(bg), B, C, c["cols"].ctypes.data, P(cols_d), nc, P(x), c["x"].shape[1], n,
                                      ge.ptr, ST())
    assert st == 0, lib.expecto_last_error()
    got = ge.result()
    print(f"B={B} nc={nc} n={n}: {int((got != c['ge']).sum())} of {got.size} counts differ")
    assert_bits(got, c["ge"], "ge")
    lut = dev_offset(c["table"], 8)
    for k_alpha, want in c["sums"].items():
        outs = [Guarded((n,), np.float64, offset=8), Guarded((n,), np.float64), Guarded((n,), np.int32, offset=4),
                Guarded((n,), np.int32)]
        assert lib.expecto_ecdf_summary(ge.ptr, n, nc, P(lut), B, k_alpha, *(o.ptr for o in outs), ST()) == 0
        for o, w, what in zip(outs, want, ("mean_nlog", "max_nlog", "top", "n_sig")):
            assert_bits(o.result(), w, f"{what} at k_alpha={k_alpha}")
    return got


@pytest.mark.parametrize("B", lengths(K))
def test_every_background_length(lib, B):
    c = case(B, 65, 130)
    got = run_both(lib, c)
    assert (got == -1).sum() == 1 and got.max() == B           # the NaN query; a query no value is below
    if B >= 4:
        assert np.isinf(c["rows"]).any() and len(np.unique(c["rows"][0])) < B     # +inf and ties in the background
        inf_q = np.isinf(c["x"][:, c["cols"]])
        assert inf_q.any() and set(got[inf_q].tolist()) <= {0, 1}                 # +inf counts the infinities


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("n", NS)
def test_variant_and_column_counts(lib, n, nc):
    c = case(K + 1, nc, n)
    run_both(lib, c)
    mean = c["sums"][1][0]
    assert np.isfinite(mean[: n // 2]).all() and (n < 2 or np.isnan(mean[n // 2]))


def test_n_sig_levels():
    c = case(K + 1, 65, 130)
    ok = (c["ge"] >= 0).all(1)
    assert (c["sums"][0][3][ok] == 0).all() and (c["sums"][K + 2][3][ok] == 65).all()
    assert np.array_equal(c["sums"][1][3][ok], (c["ge"][ok] == 0).sum(1))
    assert c["sums"][1][3][ok].max() > 0 and (c["sums"][0][3][~ok] == -1).all()


def _refusals(c):
    B, nc, n, stride = c["B"], c["nc"], c["n"], c["x"].shape[1]
    cols = c["cols"]
    swapped, far = cols.copy(), cols.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    far[-1] = C
    twice = cols.copy()
    twice[5] = twice[4]
    base = dict(bg=True, B=B, C=C, cols_host=cols, cols=True, nc=nc, x=True, stride=stride, n=n, ge=True)
    return {"B < 1": dict(base, B=0), "nc < 1": dict(base, nc=0), "nc > C": dict(base, nc=C + 1, C=C),
            "C < nc": dict(base, C=nc - 1), "not ascending": dict(base, cols_host=swapped),
            "repeated": dict(base, cols_host=twice), "out of range": dict(base, cols_host=far),
            "x_stride": dict(base, stride=int(cols.max())), "null bg": dict(base, bg=False),
            "null cols": dict(base, cols=False), "null cols_host": dict(base, cols_host=None),
            "null x": dict(base, x=False), "negative n": dict(base, n=-1)}


@pytest.mark.parametrize("bad", ["B < 1", "nc < 1", "nc > C", "C < nc", "not ascending", "repeated", "out of range",
                                 "x_stride", "null bg", "null cols", "null cols_host", "null x", "negative n"])
def test_tail_counts_refusals_write_nothing(lib, bad):
    c = case(K + 1, 65, 130)
    a = _refusals(c)[bad]
    bg, x, cols_d = device_background(c), dev_offset(c["x"], 4), dev_offset(c["cols"], 4)
    ge = Guarded((c["n"], c["nc"]), np.int32)
    lib.expecto_diff(None, None, -1, None, None)                  # another message first
    assert "negative count" in lib.expecto_last_error().decode()
    host = a["cols_host"]
    st = lib.expecto_ecdf_tail_counts(P(bg) if a["bg"] else None, a["B"], a["C"],
                                      host.ctypes.data if host is not None else None,
                                      P(cols_d) if a["cols"] else None, a["nc"], P(x) if a["x"] else None, a["stride"],
                                      a["n"], ge.ptr, ST())
    msg = lib.expecto_last_error().decode()
    assert st == EINVAL and msg and "negative count" not in msg, (bad, msg)
    assert ge.untouched()


def test_tail_counts_refuses_a_null_output_and_accepts_no_variants(lib):
    c = case(K + 1, 65, 130)
    bg, x, cols_d = device_background(c), dev_offset(c["x"], 4), dev_offset(c["cols"], 4)
    args = (P(bg), c["B"], C, c["cols"].ctypes.data, P(cols_d), c["nc"], P(x), c["x"].shape[1])
    assert lib.expecto_ecdf_tail_counts(*args, c["n"], None, ST()) == EINVAL
    assert "null" in lib.expecto_last_error().decode()
    ge = Guarded((1, c["nc"]), np.int32)
    assert lib.expecto_ecdf_tail_counts(*args, 0, ge.ptr, ST()) == 0 and ge.untouched()


@pytest.mark.parametrize("bad", ["B < 1", "nc < 1", "k_alpha > B + 1", "k_alpha < 0", "null lut", "null ge",
                                 "null output", "negative n"])
def test_summary_refusals_write_nothing(lib, bad):
    c = case(K + 1, 65, 130)
    n, nc, B = c["n"], c["nc"], c["B"]
    ge, lut = dev_offset(c["ge"], 4), dev_offset(c["table"], 8)
    outs = [Guarded((n,), np.float64), Guarded((n,), np.float64), Guarded((n,), np.int32), Guarded((n,), np.int32)]
    a = dict(ge=P(ge), n=n, nc=nc, lut=P(lut), B=B, k=1, top=outs[2].ptr)
    a.update({"B < 1": dict(B=0), "nc < 1": dict(nc=0), "k_alpha > B + 1": dict(k=B + 2), "k_alpha < 0": dict(k=-1),
              "null lut": dict(lut=None), "null ge": dict(ge=None), "null output": dict(top=None),
              "negative n": dict(n=-1)}[bad])
    lib.expecto_diff(None, None, -1, None, None)
    st = lib.expecto_ecdf_summary(a["ge"], a["n"], a["nc"], a["lut"], a["B"], a["k"], outs[0].ptr, outs[1].ptr, a["top"],
                                  outs[3].ptr, ST())
    msg = lib.expecto_last_error().decode()
    assert st == EINVAL and msg and "negative count" not in msg, (bad, msg)
    assert all(o.untouched() for o in outs)
