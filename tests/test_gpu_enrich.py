"""``expecto_cluster_enrich`` and ``expecto_hypergeom_sf`` on the device (csrc/enrich.hip), through their C
entry points, ``cluster_analysis_with_fimo.enrichment`` and the CLI.

The kernel runs one workgroup per (problem, 32 rows) with one wave per row, 64 columns and 64 bitset
words per pass; the shapes below sit on both sides of those steps, and one takes the two-wave
geometry that C = 1024 with M = 32768 needs.  Outputs lie in pattern-filled buffers (tests/guarded.py),
the contributions inside NaN margins with NaN row padding (``ld > C``).  Every count is compared
bitwise with the restatement (tests/enrich_ref.py)."""
import functools
import io
import json
import os
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch

import enrich_ref
from conftest import GOLDEN
from guarded import Guarded, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

FIMO = os.path.join(GOLDEN, "fimo")


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def caf():
    from expecto_amd import cluster_analysis_with_fimo
    return cluster_analysis_with_fimo


class Rows64:
    """float64 [V, C] on the device with row stride ld; NaN padding, NaN margins before and after."""

    def __init__(self, X, ld, margin=64):
        X = np.asarray(X, np.float64)
        n, d = X.shape
        host = np.full(margin + n * ld + margin, np.nan)
        host[margin:margin + n * ld].reshape(n, ld)[:, :d] = X
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin
        self.ld = ld


def problem(sid, rows, perm=None):
    return dict(sid=np.asarray(sid, np.int32), rows=np.asarray(rows, np.int32), perm=perm)


def as_batch(caf, problems, V, C):
    """One slot per problem for its permutation and its sid map, the row lists end to end."""
    perms = [p["perm"] for p in problems if p["perm"] is not None]
    table, off, slot = [], 0, 0
    for i, p in enumerate(problems):
        table.append((slot if p["perm"] is not None else -1, i, off, len(p["rows"])))
        slot += p["perm"] is not None
        off += len(p["rows"])
    return caf.Batch(np.array(table, np.int64).reshape(-1, 4),
                     np.stack(perms).astype(np.uint16) if perms else np.zeros((0, V, C), np.uint16),
                     np.stack([p["sid"] for p in problems]).astype(np.int32),
                     np.concatenate([p["rows"] for p in problems] + [np.zeros(0, np.int32)]).astype(np.int32))


def enrich_device(lib, caf, contrib, sets, M, matches, problems, n_neg, T, pad=3, status=0):
    """The entry point on guarded buffers -> per problem (pos_matches, pos_motifs, neg_matches, neg_motifs,
    min_rank), or the error message when ``status`` is the refusal expected."""
    contrib = np.asarray(contrib, np.float64)
    V, C = contrib.shape
    src = Rows64(contrib, C + pad)
    batch = as_batch(caf, problems, V, C)
    P = len(problems)
    bits = enrich_ref.bitsets(sets, M)
    ptr, idx = enrich_ref.csr(matches)
    S = len(matches)
    keep = [dev(bits.view(np.int64)), dev(ptr), dev(idx) if idx.size else None, dev(batch.table),
            dev(batch.perms.view(np.int16)) if batch.perms.size else None, dev(batch.sids), dev(batch.rows)]
    d_bits, d_ptr, d_idx, d_tab, d_perm, d_sid, d_rows = [None if t is None else t.data_ptr() for t in keep]
    pos_m, pos_b = Guarded((P, T), np.int64), Guarded((P, T), np.int64)
    neg, min_rank = Guarded((P, 2), np.int64), Guarded((P, C), np.int32)
    nbytes = int(lib.expecto_cluster_enrich_workspace(S, C))
    ws = Guarded((max(1, nbytes // 4),), np.int32)
    st = lib.expecto_cluster_enrich(src.ptr, V, C, src.ld, d_bits, M, ptr.ctypes.data, d_ptr, d_idx, S,
                                    batch.table.ctypes.data, d_tab, P, d_perm, batch.perms.shape[0], d_sid,
                                    batch.sids.shape[0], d_rows, batch.rows.shape[0], n_neg, T, pos_m.ptr, pos_b.ptr,
                                    neg.ptr, min_rank.ptr, ws.ptr, max(nbytes, 4), ST())
    torch.cuda.synchronize()
    if status != 0:
        assert st == status
        assert pos_m.untouched() and pos_b.untouched() and neg.untouched() and min_rank.untouched()
        return lib.expecto_last_error().decode()
    assert st == 0, lib.expecto_last_error().decode()
    ws.result()
    pos_m, pos_b, neg, min_rank = pos_m.result(), pos_b.result(), neg.result(), min_rank.result()
    return [(pos_m[p], pos_b[p], neg[p, 0], neg[p, 1], min_rank[p]) for p in range(P)]


def assert_counts(got, want, what):
    for g, w, name in zip(got, want, ("pos_matches", "pos_motifs", "neg_matches", "neg_motifs", "min_rank")):
        assert_bits(np.asarray(g), np.asarray(w), f"{what} {name}")


def reference(contrib, sets, matches, problems, n_neg, T):
    return [enrich_ref.counts(contrib, sets, matches, p["sid"], p["rows"], n_neg, T, perm=p["perm"]) for p in problems]


@functools.lru_cache(maxsize=None)
def case(V, C, M, S, seed=0, ties=False):
    """Random contributions, sets of up to 5 motifs that overlap, match lists with repeats and empty
    lists, a sid map with -1 and shared sequences.  ``ties``: magnitudes from {0, 1, 2} with both signs."""
    rng = np.random.RandomState(1000 + seed)
    if ties:
        contrib = rng.randint(-2, 3, (V, C)).astype(np.float64)
        contrib[0] = 0.0
        contrib[contrib == 0] *= rng.choice([1.0, -1.0], int((contrib == 0).sum()))      # +0.0 and -0.0
    else:
        contrib = rng.standard_normal((V, C))
    sets = tuple(frozenset(rng.randint(0, M, rng.randint(1, 6)).tolist()) | ({M - 1} if c % 3 == 0 else set())
                 for c in range(C))
    matches = tuple(tuple(rng.randint(0, M, rng.randint(0, 12)).tolist()) if s % 4 != 3 else () for s in range(S))
    sid = rng.randint(-1, S, V).astype(np.int32)
    contrib.setflags(write=False)
    return contrib, [set(s) for s in sets], [list(m) for m in matches], sid


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("ends", ["1_1", "C_C", "1_C", "C_1"])
def test_counts_at_the_column_edges(lib, caf, C, ends):
    n_neg, T = [1 if e == "1" else C for e in ends.split("_")]
    contrib, sets, matches, sid = case(7, C, 65, 5)
    probs = [problem(sid, np.arange(7))]
    got = enrich_device(lib, caf, contrib, sets, 65, matches, probs, n_neg, T)
    assert_counts(got[0], reference(contrib, sets, matches, probs, n_neg, T)[0], f"C={C} n_neg={n_neg} T={T}")


@pytest.mark.parametrize("M", [1, 64, 65, 129])
def test_counts_at_the_bitset_word_edges(lib, caf, M):
    contrib, sets, matches, sid = case(6, 5, M, 4, seed=1)
    assert any(M - 1 in s for s in sets)
    probs = [problem(sid, np.arange(6))]
    got = enrich_device(lib, caf, contrib, sets, M, matches, probs, 2, 3)
    assert_counts(got[0], reference(contrib, sets, matches, probs, 2, 3)[0], f"M={M}")


@pytest.mark.parametrize("V", [1, 70])
def test_one_row_and_more_than_one_workgroup(lib, caf, V):
    contrib, sets, matches, sid = case(V, 9, 70, 6, seed=2)
    probs = [problem(sid, np.arange(V))]
    got = enrich_device(lib, caf, contrib, sets, 70, matches, probs, 3, 6)
    assert_counts(got[0], reference(contrib, sets, matches, probs, 3, 6)[0], f"V={V}")


def test_two_wave_geometry(lib, caf):
    """C = 1024 with M = 32768 and T = C needs more than 64 KiB of LDS at four waves: two are launched."""
    contrib, sets, matches, sid = case(3, 1024, 32768, 3, seed=3)
    probs = [problem(sid, np.arange(3))]
    got = enrich_device(lib, caf, contrib, sets, 32768, matches, probs, 1024, 1024)
    assert_counts(got[0], reference(contrib, sets, matches, probs, 1024, 1024)[0], "C=1024")


def test_rows_without_sequence_empty_lists_and_shared_sequences(lib, caf):
    contrib, sets, _, _ = case(5, 6, 20, 3, seed=4)
    matches = [[0, 0, 3, 19], [], [7, 7, 7]]             # repeats count; sequence 1 is empty
    sid = np.array([0, -1, 1, 0, 2], np.int32)           # rows 0 and 3 share a sequence, row 1 has none
    probs = [problem(sid, np.arange(5)), problem(np.full(5, -1), np.arange(5))]
    got = enrich_device(lib, caf, contrib, sets, 20, matches, probs, 2, 4)
    want = reference(contrib, sets, matches, probs, 2, 4)
    for p in range(2):
        assert_counts(got[p], want[p], f"problem {p}")
    assert got[1][0].sum() == 0 and got[1][2] == 0 and got[1][1].sum() > 0       # motifs are still counted


def test_bottom_set_is_a_union(lib, caf):
    """Motif 5 sits in both bottom clusters and matches twice: 2 matches of 3 motifs, not 4 of 4."""
    contrib = np.array([[3.0, -2.0, 1.0, 0.5]])
    sets = [{0}, {1}, {5, 6}, {5, 7}]
    got = enrich_device(lib, caf, contrib, sets, 8, [[5, 5, 0]], [problem([0], [0])], 2, 2)[0]
    assert got[0].tolist() == [1, 0] and got[1].tolist() == [1, 1]
    assert (int(got[2]), int(got[3])) == (2, 3)
    assert got[4].tolist() == [0, 1, 2, 3]


def test_ties_take_the_lower_column_first(lib, caf):
    contrib, sets, matches, sid = case(9, 70, 65, 5, seed=5, ties=True)
    assert (contrib[0] == 0).all() and (np.signbit(contrib[contrib == 0])).any()
    probs = [problem(sid, np.arange(9))]
    got = enrich_device(lib, caf, contrib, sets, 65, matches, probs, 7, 70)
    assert_counts(got[0], reference(contrib, sets, matches, probs, 7, 70)[0], "ties")
    # +x / -x: columns 0 and 1 tie, column 2 is larger
    one = enrich_device(lib, caf, np.array([[-1.0, 1.0, 2.0], [0.0, -0.0, 0.0]]), [{0}, {1}, {2}], 3, [[0]],
                        [problem([0, -1], [0]), problem([0, -1], [1])], 1, 3)
    assert one[0][4].tolist() == [1, 2, 0] and one[0][0].tolist() == [0, 1, 0]
    assert one[1][4].tolist() == [0, 1, 2]


def test_a_mixed_batch_equals_its_problems_alone(lib, caf):
    V, C = 40, 11
    contrib, sets, matches, sid = case(V, C, 100, 7, seed=6)
    rng = np.random.RandomState(9)
    perm = lambda: rng.rand(V, C).argsort(axis=1).astype(np.uint16)
    probs = [problem(sid, np.arange(V)), problem(sid, np.arange(V), perm()), problem(sid[rng.permutation(V)], np.arange(V)),
             problem(sid, [3, 5, 39]), problem(sid[::-1].copy(), np.arange(33), perm()), problem(sid, []),
             problem(sid, [7])]
    got = enrich_device(lib, caf, contrib, sets, 100, matches, probs, 4, 6)
    want = reference(contrib, sets, matches, probs, 4, 6)
    for p, pr in enumerate(probs):
        assert_counts(got[p], want[p], f"batch problem {p}")
        if len(pr["rows"]):
            assert_counts(enrich_device(lib, caf, contrib, sets, 100, matches, [pr], 4, 6)[0], got[p], f"alone {p}")
    assert got[5][4].tolist() == [C] * C and got[5][1].sum() == 0          # no rows: nothing ranked


def test_refusals(lib, caf):
    contrib, sets, matches, sid = case(4, 5, 10, 3, seed=7)
    probs = [problem(sid, np.arange(4))]
    bad = np.array(contrib)
    bad[2, 4] = np.nan
    assert "NaN" in enrich_device(lib, caf, bad, sets, 10, matches, probs, 2, 2, status=-1)
    assert "n_neg" in enrich_device(lib, caf, contrib, sets, 10, matches, probs, 6, 2, status=-1)
    assert "T must" in enrich_device(lib, caf, contrib, sets, 10, matches, probs, 2, 6, status=-1)
    assert lib.expecto_cluster_enrich(None, 4, 1025, 1025, None, 10, None, None, None, 3, None, None, 1, None, 0, None,
                                      1, None, 4, 2, 2, None, None, None, None, None, 0, ST()) == -1
    assert "[1, 1024]" in lib.expecto_last_error().decode()
    # zero problems: success, nothing written
    pos = Guarded((1, 2), np.int64)
    assert lib.expecto_cluster_enrich(None, 4, 5, 5, None, 10, None, None, None, 3, None, None, 0, None, 0, None, 0,
                                      None, 0, 2, 2, pos.ptr, pos.ptr, pos.ptr, pos.ptr, None, 0, ST()) == 0
    torch.cuda.synchronize()
    assert pos.untouched()


# ---- expecto_hypergeom_sf ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def quadruples():
    """``enrich_ref.sf_quadruples()`` with their exact tails (tests/golden/fimo/hypergeom_exact.json: 40
    digits, computed once by make_golden_fimo.py)."""
    rows = json.load(open(os.path.join(FIMO, "hypergeom_exact.json")))
    assert [tuple(r[:4]) for r in rows] == enrich_ref.sf_quadruples()
    return np.array([r[:4] for r in rows], np.int64), [None if r[4] is None else Fraction(r[4]) for r in rows]


def relative_errors(values, exact):
    """Largest relative error over the cases whose exact value is a normal double, and the count of them."""
    worst, used = 0.0, 0
    for v, e in zip(values, exact):
        if e is None or not 2.3e-308 < float(e) < np.inf:
            continue
        worst = max(worst, float(abs(Fraction(float(v)) - e) / e))
        used += 1
    return worst, used


def sf_device(lib, q):
    d = dev(np.ascontiguousarray(q.T))
    out = Guarded((q.shape[0],), np.float64)
    st = lib.expecto_hypergeom_sf(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), q.shape[0], out.ptr,
                                  ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    return out.result()


def test_hypergeom_sf_against_the_exact_tail(lib):
    """The device's largest relative error may be at most twice scipy's on the same cases; both are
    measured against the exact rational tail.  Measured on an MI355X: device 4.98e-14, scipy 1.15e-10
    (with the anchor term from lgamma the device had 2.9e-9 and missed this bound)."""
    from scipy.stats import hypergeom
    q, exact = quadruples()
    got = sf_device(lib, q)
    ref = hypergeom.sf(q[:, 0] - 1, q[:, 1], q[:, 2], q[:, 3])
    for g, e, (k, M, n, N) in zip(got, exact, q.tolist()):      # the branches without arithmetic are exact
        if e is None:
            assert np.isnan(g)
        elif k <= max(0, N - (M - n)) or k > min(n, N):
            assert e in (0, 1) and g == float(e)
    assert np.isnan(ref[[e is None for e in exact]]).all()
    err_dev, used = relative_errors(got, exact)
    err_ref, _ = relative_errors(ref, exact)
    print(f"hypergeom_sf: {used} cases, largest relative error device {err_dev:.3e}, scipy {err_ref:.3e}")
    for v, r, e, x in zip(got, ref, exact, q.tolist()):
        if e is not None and 2.3e-308 < float(e) and abs(Fraction(float(v)) - e) / e > 1e-13:
            print("  ", x, f"device {float(abs(Fraction(float(v)) - e) / e):.3e} scipy {float(abs(Fraction(float(r)) - e) / e):.3e}")
    assert used >= 200 and min(float(e) for e in exact if e and float(e) > 2.3e-308) < 1e-290
    assert err_dev <= 2 * err_ref, (err_dev, err_ref)
    assert lib.expecto_hypergeom_sf(None, None, None, None, 0, None, ST()) == 0
    assert lib.expecto_hypergeom_sf(None, None, None, None, 3, None, ST()) == -1


# ---- end to end ----------------------------------------------------------------------------------

def cli_args(caf, name, out_dir, *extra):
    d = os.path.join(FIMO, name)
    return caf.build_parser().parse_args(["--cluster_contribs_file", os.path.join(d, "cluster_contribs.tsv"),
                                          "--rsat_clusters_file", os.path.join(d, "rsat_clusters.tsv"),
                                          "--fimo_out_file", os.path.join(d, "fimo.tsv"), "-o", str(out_dir), *extra])


@pytest.mark.parametrize("name,extra,golden", [("main", (), "stdout.txt"), ("shared", (), "stdout.txt"),
                                               ("main", ("--rank_int",), "stdout_rank_int.txt")])
def test_cli_gives_the_golden_stdout(lib, caf, tmp_path, name, extra, golden):
    """Line for line; a p-value as a parsed float within twice the error measured for scipy on the
    quadruples above (the golden digits are scipy's), the bound of the test before this one."""
    from scipy.stats import hypergeom
    q, exact = quadruples()
    tol = 3 * relative_errors(hypergeom.sf(q[:, 0] - 1, q[:, 1], q[:, 2], q[:, 3]), exact)[0]   # ours 2x + theirs 1x
    out = io.StringIO()
    res, _ = caf.run(cli_args(caf, name, tmp_path, *extra), out=out)
    got, want = out.getvalue().splitlines(), open(os.path.join(FIMO, name, golden)).read().splitlines()
    assert len(got) == len(want) == 43 and got[-1] == want[-1] == "end"
    for g, w in zip(got[:-1], want[:-1]):
        (gh, gp), (wh, wp) = g.rsplit(": ", 1), w.rsplit(": ", 1)
        assert gh == wh
        assert abs(float(gp) - float(wp)) <= tol * float(wp), (g, w)
    # hypergeom.tsv holds the restatement's integers
    inp = caf.load(cli_args(caf, name, tmp_path, *extra), np.random.RandomState(1))
    rs = np.random.RandomState(1)
    if extra:
        caf.load(cli_args(caf, name, tmp_path, *extra), rs)
    batch = caf.reference_batch(inp, *next(caf.draw_shuffles(rs, 12, 25, 1)))
    ptr, idx = caf.csr(inp.matches)
    pm, pb, neg, mr = enrich_ref.counts_batch(inp.contrib, caf.bitsets(inp.sets, len(inp.motifs)), len(inp.motifs), ptr,
                                              idx, batch, 20, 6)
    tsv = pd.read_csv(tmp_path / "hypergeom.tsv", sep="\t")
    assert tsv["problem"].tolist() == [p for p in caf.PROBLEMS for _ in range(6)]
    assert_bits(tsv["k"].to_numpy(np.int64).reshape(7, 6), pm, "k")
    assert_bits(tsv["n"].to_numpy(np.int64).reshape(7, 6), pb, "n")
    assert_bits(tsv["M"].to_numpy(np.int64).reshape(7, 6), pb + neg[:, 1:2], "M")
    assert_bits(tsv["N"].to_numpy(np.int64).reshape(7, 6), pm + neg[:, 0:1], "N")
    assert_bits(res.min_rank, mr, "min_rank")
    uniq = pd.read_csv(tmp_path / "num_unique_clusters.tsv", sep="\t")["n_unique_clusters"].to_numpy(np.int64)
    assert_bits(uniq, enrich_ref.n_unique(mr[0], 6), "n_unique")


def test_permutations_leave_the_reference_problems(lib, caf, tmp_path, monkeypatch):
    """--n_permutations 3, in chunks of one permutation: the seven problems are bit-equal to a run
    without, and null row j equals a single run of permutation j."""
    one, none = caf.run(cli_args(caf, "main", tmp_path / "a"), out=io.StringIO())
    monkeypatch.setattr(caf, "PERM_BYTES", 1)
    monkeypatch.setattr(caf, "chunk_size", lambda V, C, budget=1: 1)
    three, null = caf.run(cli_args(caf, "main", tmp_path / "b", "--n_permutations", "3"), out=io.StringIO())
    assert none is None and null.shape == (2, 3, 6)
    for a, b in zip(one, three):
        assert_bits(a, b, "reference problems")
    assert_bits(null[:, 0], one.pval[1:3], "null row 0")
    inp = caf.load(cli_args(caf, "main", tmp_path))
    draws = list(caf.draw_shuffles(np.random.RandomState(1), 12, 25, 3))
    for j in (1, 2):
        single = caf.enrichment(inp.contrib, inp.sets, inp.matches, caf.permutation_batch(inp, [draws[j]]), 20, 6,
                                n_motifs=len(inp.motifs))
        assert_bits(single.pval, null[:, j], f"null row {j}")
    timings = {"sf_ms": 1e9}
    both = caf.enrichment(torch.from_numpy(inp.contrib).cuda(), caf.bitsets(inp.sets, len(inp.motifs)),
                          caf.csr(inp.matches), caf.permutation_batch(inp, draws[1:]), 20, 6, n_motifs=len(inp.motifs),
                          timings=timings)
    assert_bits(both.pval[0::2], null[0, 1:], "device tensor, clusters")
    assert_bits(both.pval[1::2], null[1, 1:], "device tensor, variants")
    assert set(timings) == {"upload_ms", "enrich_ms", "sf_ms"}
    assert all(isinstance(v, float) and np.isfinite(v) and v >= 0 for v in timings.values())
    assert timings["sf_ms"] >= 1e9                                     # these keys accumulate over calls
    assert os.path.exists(tmp_path / "b" / "permutation_null.tsv")
