"""CPU: the attribution step (predict_by_cluster[_rsat].py drop-in) -- the numpy restatements of
tests/contrib_ref.py against the reference's own outputs (tests/golden/make_golden_contribs.py)
and against each other, and the host-side parsing of expecto_amd.predict_by_cluster."""
import os

import numpy as np
import pandas as pd
import pytest

import contrib_ref
from conftest import GOLDEN

PBC = os.path.join(GOLDEN, "predict_by_cluster")
FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
BASE_COLUMNS = 13      # index, 0-4, dist, gene, strand, REF, ALT, SED, SED_PROPORTION; then the contributions


def golden_table(name):
    df = pd.read_csv(os.path.join(PBC, name), sep="\t", float_precision="round_trip")
    return df.sort_values("index").reset_index(drop=True)


@pytest.fixture(scope="module")
def golden_case():
    return contrib_ref.golden_inputs(GOLDEN)


def test_keep_mask_of_the_synthetic_lambert_tables(golden_case):
    h = golden_case["hgnc"]
    assert len(golden_case["keep"]) == 40
    assert h["Assay"].value_counts().to_dict() == {"MAX": 9, "JUN": 9, "FOS": 8, "ZNF274": 7, "STAT3": 7}
    assert golden_case["not_found"] == {"STAT3"}


def test_dump_weights_are_the_dump_lines(tmp_path):
    from expecto_amd.xgblinear import GBLinear
    m = GBLinear.load(os.path.join(PBC, "model.save"))
    m.save_dump(str(tmp_path / "m.txt"))
    lines = open(tmp_path / "m.txt").read().strip("\n").split("\n")
    assert lines[:2] == ["booster[0]:", "bias:"] and lines[3] == "weight:"
    w = m.dump_weights()
    assert w.dtype == np.float64 and np.array_equal(w, np.array(list(map(float, lines[4:]))))
    assert not np.array_equal(w, m.weights[:, 0].astype(np.float64))      # %g keeps 6 digits


def test_reference_order_reproduces_the_golden_columns(golden_case):
    g = golden_case
    r = contrib_ref.reference_order(g["weights"], g["ref"], g["alt"], g["assay_clusters"])
    want = golden_table("sed_sorted_by_proportion_with_contribs.tsv")
    assert want.shape[1] == BASE_COLUMNS + 40
    header = open(os.path.join(PBC, "sed_sorted_by_proportion_with_contribs.tsv")).readline().rstrip("\n").split("\t")
    assert header[BASE_COLUMNS:] == (g["hgnc"]["Assay"] + "/" + g["hgnc"]["Cell type"]).tolist()
    assert np.array_equal(want.iloc[:, -40:].to_numpy(), r["prop"])
    wantc = golden_table("cluster_contribs.tsv")
    names = [f"cluster_{i}" for i in r["columns"]]
    assert list(wantc.columns[-len(names):]) == names == ["cluster_1", "cluster_2", "cluster_3", "cluster_-1"]
    assert np.array_equal(wantc[names].to_numpy(), r["clu_prop"])


def test_golden_sed_proportions_are_distinct(golden_case):
    """The sorted files' row order is decided by SED_PROPORTION: its golden values differ by far
    more than float32 scoring noise (1e-5 relative, tests/test_gpu_predict.py), so the device run
    must reproduce the order."""
    p = np.sort(golden_table("cluster_contribs.tsv")["SED_PROPORTION"].to_numpy())
    assert np.all(np.diff(p) > 1e-3 * p[1:])


def seeded(seed, n, nk, n_models=1):
    rng = np.random.default_rng(seed)
    ref = rng.normal(0, 1, (n, 10 * nk))
    alt = ref + rng.normal(0.05, 0.1, (n, 10 * nk))
    # differences and weights of a preferred sign keep |total| well above 1e-3 * sum |contrib|
    w = np.array([[float("%g" % x) for x in row] for row in rng.normal(0.05, 0.02, (n_models, 10 * nk))])
    return ref, alt, w


def marks_of(columns, assay_clusters):
    return [[f for f, ids in enumerate(assay_clusters) if c in ids] for c in columns]


@pytest.mark.parametrize("nk,seed", [(40, 1), (257, 2), (2002, 3)])
def test_device_order_is_within_the_derived_bounds_of_reference_order(nk, seed):
    n = 5
    ref, alt, w = seeded(seed, n, nk)
    rng = np.random.default_rng(100 + seed)
    assay_clusters = [sorted(set(rng.integers(1, 6, rng.integers(1, 3)).tolist())) for _ in range(nk)]
    assay_clusters[0] = [1, 2]                      # a mark in two clusters
    assay_clusters[-1] = [-1]
    r = contrib_ref.reference_order(w[0], ref, alt, assay_clusters)
    members = marks_of(r["columns"], assay_clusters)
    d = contrib_ref.device_order(ref, alt, nk, np.arange(nk), w, members)
    b = contrib_ref.bounds(w[0], ref, alt, r, members)
    assert b["prop_rows"].all() and b["clu_rows"].all()       # no row is left out of the proportion checks
    for key in ("contrib", "total", "prop", "clu", "clu_prop"):
        err = np.abs(d[key][0] - r[key])
        assert np.all(err <= b[key]), (key, float((err / np.maximum(b[key], 1e-300)).max()))


def test_device_order_single_label_clusters_against_groupby():
    nk, n = 64, 4
    ref, alt, w = seeded(7, n, nk)
    labels = pd.Series(np.random.default_rng(8).integers(0, 5, nk))
    r = contrib_ref.reference_order(w[0], ref, alt, labels)
    members = [np.nonzero(labels.to_numpy() == c)[0].tolist() for c in sorted(set(labels))]
    d = contrib_ref.device_order(ref, alt, nk, np.arange(nk), w, members)
    b = contrib_ref.bounds(w[0], ref, alt, r, members)
    assert b["clu_rows"].all()
    for key in ("clu", "clu_prop"):
        assert np.all(np.abs(d[key][0] - r[key]) <= b[key]), key


def test_wave_sum_order():
    x = np.random.default_rng(0).normal(0, 1, 200)
    lanes = [x[l::64] for l in range(64)]
    p = [float(np.add.reduce(v[:1])) if len(v) else -0.0 for v in lanes]
    for l, v in enumerate(lanes):
        for y in v[1:]:
            p[l] = p[l] + y
    for s in (32, 16, 8, 4, 2, 1):
        p = [p[l] + p[l + s] for l in range(s)]
    assert contrib_ref.wave_sum(x) == p[0]
    assert contrib_ref.wave_sum(np.zeros(0)) == 0.0 and not np.signbit(contrib_ref.wave_sum(np.zeros(0)))
    assert np.signbit(contrib_ref.wave_sum(np.array([-0.0, -0.0])))


def test_rsat_tab_parsing(tmp_path, golden_case):
    from expecto_amd import predict_by_cluster as pbc
    ids, table = pbc.rsat_clusters(os.path.join(PBC, "clusters_motif_names.tab"), golden_case["hgnc"]["Assay"])
    assert ids == golden_case["assay_clusters"]
    by_assay = dict(zip(golden_case["hgnc"]["Assay"], ids))
    assert by_assay == {"MAX": [1, 2], "JUN": [2], "FOS": [2], "ZNF274": [3], "STAT3": [-1]}
    table.to_csv(tmp_path / "rsat_clusters.tsv", sep="\t", header=None)
    assert open(tmp_path / "rsat_clusters.tsv").read() == open(os.path.join(PBC, "rsat_clusters.tsv")).read()
    cluster_ids, members = pbc.clusters_from_assay_ids(ids)
    assert cluster_ids == [1, 2, 3, -1]            # cluster 4 (TP53) holds no kept mark: no column
    assert sorted(members[0] + members[3] + members[2]) == [f for f, a in enumerate(golden_case["hgnc"]["Assay"])
                                                           if a in ("MAX", "STAT3", "ZNF274")]
    assert set(members[0]) <= set(members[1])      # MAX sits in clusters 1 and 2


def test_feature_clusters_parsing(tmp_path):
    from expecto_amd import predict_by_cluster as pbc
    labels = np.array([2, 0, 2, 5])
    per_coeff = pd.DataFrame({"Assay": np.repeat(list("abcd"), 10), "coeff_idx": np.tile(np.arange(10), 4),
                              "cluster": np.repeat(labels, 10)})
    per_coeff.to_csv(tmp_path / "all_feature_clusters.tsv", sep="\t")
    assert pbc.feature_clusters(str(tmp_path / "all_feature_clusters.tsv"), 4) == ([0, 2, 5], [[1], [0, 2], [3]])
    per_coeff.iloc[::10].to_csv(tmp_path / "per_mark.tsv", sep="\t")
    assert pbc.feature_clusters(str(tmp_path / "per_mark.tsv"), 4) == ([0, 2, 5], [[1], [0, 2], [3]])
    per_coeff.loc[3, "cluster"] = 1
    per_coeff.to_csv(tmp_path / "mixed.tsv", sep="\t")
    with pytest.raises(ValueError, match="different labels"):
        pbc.feature_clusters(str(tmp_path / "mixed.tsv"), 4)
    with pytest.raises(ValueError, match="kept marks"):
        pbc.feature_clusters(str(tmp_path / "per_mark.tsv"), 5)


def test_multi_model_output_layout_and_arguments():
    from expecto_amd import predict_by_cluster as pbc
    assert pbc.model_dirs("out", ["a/m1.save"]) == ["out"]
    assert pbc.model_dirs("out", ["a/m1.save", "b/m2.txt"]) == [os.path.join("out", "m1"), os.path.join("out", "m2")]
    with pytest.raises(ValueError, match="distinct"):
        pbc.model_dirs("out", ["a/m.save", "b/m.save"])
    args = pbc.build_parser().parse_args(["--model_save_file", "x.save", "y.save", "--rsat_clusters_tab", "t.tab",
                                          "--coorFile_chromatin", "c.vcf", "-o", "o"])
    assert args.model_save_file == ["x.save", "y.save"] and args.feature_clusters_df is None
    with pytest.raises(ValueError, match="intersect_with_lambert"):
        pbc.run(args)
    args = pbc.build_parser().parse_args(["--model_save_file", "x.save", "-o", "o"])
    with pytest.raises(ValueError, match="one of"):
        pbc.run(args)


def test_clusters_csr_checks_members():
    from expecto_amd.features import clusters_csr
    ptr, mark = clusters_csr([[0, 2], [], [2]], 3)
    assert ptr.tolist() == [0, 2, 2, 3] and mark.tolist() == [0, 2, 2]
    with pytest.raises(RuntimeError, match="kept marks"):
        clusters_csr([[3]], 3)
