"""CPU: the restatement of tests/enrich_ref.py is anchored to the reference's golden stdout
(tests/golden/fimo, written by tests/golden/make_golden_fimo.py), and the host half of
``expecto_amd.cluster_analysis_with_fimo`` (reading, filtering, the seven problems, the draws) is checked
with the device calls replaced by the restatement and scipy."""
import io
import os
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import enrich_ref
from conftest import GOLDEN
from expecto_amd import cluster_analysis_with_fimo as caf

FIMO = os.path.join(GOLDEN, "fimo")


def cli_args(case, out_dir, *extra):
    d = os.path.join(FIMO, case)
    return caf.build_parser().parse_args(["--cluster_contribs_file", os.path.join(d, "cluster_contribs.tsv"),
                                          "--rsat_clusters_file", os.path.join(d, "rsat_clusters.tsv"),
                                          "--fimo_out_file", os.path.join(d, "fimo.tsv"), "-o", str(out_dir), *extra])


def scipy_sf(k, M, n, N, device=None, timings=None):
    from scipy.stats import hypergeom
    return np.asarray(hypergeom.sf(np.asarray(k) - 1, M, n, N), np.float64)


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(caf, "device_counts", enrich_ref.counts_batch)
    monkeypatch.setattr(caf, "device_sf", scipy_sf)


@pytest.mark.parametrize("case,extra,golden", [("main", (), "stdout.txt"), ("shared", (), "stdout.txt"),
                                               ("main", ("--rank_int",), "stdout_rank_int.txt")])
def test_restatement_reproduces_the_reference_stdout(host_only, tmp_path, case, extra, golden):
    """Every printed digit: the restatement's integers through scipy's hypergeom.sf, for the data, both
    shuffles (so the draws and, with --rank_int, the stream rank_INT leaves) and the four quartiles."""
    out = io.StringIO()
    caf.run(cli_args(case, tmp_path, *extra), out=out)
    want = open(os.path.join(FIMO, case, golden)).read()
    assert want.count("Top cluster index") == 7 * 6
    assert out.getvalue() == want


def test_fixture_files_are_the_recipe():
    for case in ("main", "shared"):
        for name, text in zip(("cluster_contribs.tsv", "rsat_clusters.tsv", "fimo.tsv"), enrich_ref.fixture(case)):
            assert open(os.path.join(FIMO, case, name)).read() == text, (case, name)


def test_filter_and_problem_construction(tmp_path):
    args = cli_args("main", tmp_path)
    inp = caf.load(args)
    df = pd.read_csv(args.cluster_contribs_file, sep="\t", index_col=0)
    V, C = 12, 25
    assert inp.contrib.shape == (V, C) and inp.columns == [f"cluster_{c + 1}" for c in range(C)]
    assert inp.n_cluster_rows == 26 and len(inp.motifs) == 77          # 75 placed + the two of cluster_-1
    np.testing.assert_array_equal(inp.contrib, df[inp.columns].to_numpy())
    np.testing.assert_array_equal(inp.sed, df["SED_PROPORTION"].to_numpy())

    # the filter: window around position 31, best row per (motif_id, motif_alt_id, sequence), threshold
    fimo = pd.read_table(args.fimo_out_file, sep="\t", names=caf.FIMO_COLUMNS, comment="#")
    kept = {}
    for r in fimo.itertuples(index=False):
        if r.start <= 31 <= r.stop:
            key = (r.motif_id, r.motif_alt_id, r.sequence_name)
            kept[key] = min(kept.get(key, np.inf), r[7])
    want = {}
    for (_, motif, seq), p in kept.items():
        if p < 1e-4:
            want.setdefault(seq, []).append(inp.motifs.index(motif))
    assert 0 < sum(map(len, want.values())) < len(fimo)                 # some rows fall to each filter
    assert set(inp.sequences) == set(want)
    for s, name in enumerate(inp.sequences):
        assert sorted(inp.matches[s]) == sorted(want[name]), name
    for v, rsid in enumerate(df["2"].tolist()):
        assert inp.sid[v] == (inp.sequences.index(rsid) if rsid in want else -1)
    assert (inp.sid == -1).any() and "rs_elsewhere" in inp.sequences

    # the draws: the legacy global stream after seed(1), in the reference's order
    rs = np.random.RandomState(1)
    draws = list(caf.draw_shuffles(rs, V, C, 3))
    np.random.seed(1)
    for idx, random_idxs in draws:
        np.testing.assert_array_equal(idx, np.random.rand(V, C).argsort(axis=1))
        np.testing.assert_array_equal(random_idxs, np.random.choice(V, V, replace=False))

    batch = caf.reference_batch(inp, *draws[0])
    assert batch.table.shape == (7, 4) and batch.table[:, 0].tolist() == [-1, 0, -1, -1, -1, -1, -1]
    np.testing.assert_array_equal(np.take_along_axis(inp.contrib, batch.perms[0].astype(np.int64), 1),
                                  np.take_along_axis(inp.contrib, draws[0][0].astype(np.int64), 1))
    np.testing.assert_array_equal(batch.sids[0], inp.sid)
    np.testing.assert_array_equal(batch.sids[1], inp.sid[draws[0][1]])
    sed = inp.sed
    for q, (a, b) in enumerate(caf.PERCENTILES):
        off, cnt = batch.table[3 + q, 2:]
        lo, hi = np.percentile(sed, a), np.percentile(sed, b)
        assert batch.rows[off:off + cnt].tolist() == [v for v in range(V) if lo <= sed[v] <= hi]
        assert 3 <= cnt <= 4
    more = caf.permutation_batch(inp, draws[1:])
    assert more.table.tolist() == [[0, 0, 0, V], [-1, 1, 0, V], [1, 0, 0, V], [-1, 2, 0, V]]
    np.testing.assert_array_equal(more.sids[2], inp.sid[draws[2][1]])
    np.testing.assert_array_equal(more.perms[1], draws[2][0])


def test_shared_motif_sits_in_two_sets(tmp_path):
    inp = caf.load(cli_args("shared", tmp_path))
    m = inp.motifs.index("M00a_HUMAN.H11MO.0.A")
    assert m in inp.sets[0] and m in inp.sets[1] and len(inp.sets[1]) == 4


def test_permutations_extend_the_reference_run(host_only, tmp_path):
    """--n_permutations 3: the seven problems stay, null row j is permutation j alone, and the files."""
    one, none = caf.run(cli_args("main", tmp_path / "a"), out=io.StringIO())
    three, null = caf.run(cli_args("main", tmp_path / "b", "--n_permutations", "3"), out=io.StringIO())
    assert none is None and null.shape == (2, 3, 6)
    np.testing.assert_array_equal(one.pval, three.pval)
    np.testing.assert_array_equal(null[:, 0], one.pval[1:3])
    inp = caf.load(cli_args("main", tmp_path))
    draws = list(caf.draw_shuffles(np.random.RandomState(1), 12, 25, 3))
    for j in (1, 2):
        single = caf.enrichment(inp.contrib, inp.sets, inp.matches, caf.permutation_batch(inp, [draws[j]]), 20, 6,
                                n_motifs=len(inp.motifs))
        np.testing.assert_array_equal(single.pval, null[:, j])
    table = pd.read_csv(tmp_path / "b" / "permutation_null.tsv", sep="\t")
    assert len(table) == 12 and not os.path.exists(tmp_path / "a" / "permutation_null.tsv")
    emp = (1 + (null[0] <= one.pval[0]).sum(0)) / 4.0
    np.testing.assert_array_equal(table["empirical_pval"].to_numpy()[:6], emp)
    hyp = pd.read_csv(tmp_path / "b" / "hypergeom.tsv", sep="\t")
    assert hyp["problem"].tolist() == [p for p in caf.PROBLEMS for _ in range(6)]
    np.testing.assert_array_equal(hyp["k"].to_numpy().reshape(7, 6), one.k)
    uniq = pd.read_csv(tmp_path / "b" / "num_unique_clusters.tsv", sep="\t")["n_unique_clusters"].to_numpy()
    np.testing.assert_array_equal(uniq, enrich_ref.n_unique(one.min_rank[0], 6))
    assert (np.diff(uniq) >= 0).all() and uniq[0] >= 1


def test_chunk_size_follows_the_byte_budget():
    assert caf.chunk_size(5000, 110) == (256 << 20) // (2 * 5000 * 110 + 4 * 5000)
    assert caf.chunk_size(5000, 110, budget=1) == 1


def test_refusals_before_the_device(tmp_path):
    inp = caf.load(cli_args("main", tmp_path))
    batch = caf.reference_batch(inp, *next(caf.draw_shuffles(np.random.RandomState(1), 12, 25, 1)))
    for kw, text in ((dict(n_neg=26, T=6), "n_neg"), (dict(n_neg=20, T=26), "T = 26")):
        with pytest.raises(ValueError, match=text):
            caf.enrichment(inp.contrib, inp.sets, inp.matches, batch, n_motifs=77, **kw)
    bad = inp.contrib.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        caf.enrichment(bad, inp.sets, inp.matches, batch, 20, 6, n_motifs=77)
    # a cluster row that no column names: 27 rows less 1 leave 26 indices for 25 columns (an IndexError there)
    args = cli_args("main", tmp_path, "--n_neg_clusters", "1")
    rows = open(args.rsat_clusters_file).read().splitlines()
    rows.insert(25, "cluster_99\tM00a_HUMAN.H11MO.0.A")
    args.rsat_clusters_file = str(tmp_path / "rsat_clusters.tsv")
    open(args.rsat_clusters_file, "w").write("\n".join(rows) + "\n")
    with pytest.raises(ValueError, match="only 25 cluster columns"):
        caf.run(args, out=io.StringIO())


def test_exact_tail():
    assert enrich_ref.exact_sf(4, 10, 8, 5) == Fraction(7, 9)
    assert enrich_ref.exact_sf(0, 10, 5, 5) == 1 and enrich_ref.exact_sf(6, 10, 5, 5) == 0
    assert enrich_ref.exact_sf(1, 0, 0, 0) is None and enrich_ref.exact_sf(3, 10, 12, 5) is None
