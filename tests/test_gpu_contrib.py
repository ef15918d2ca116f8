"""GPU: expecto_variant_contrib BIT FOR BIT against tests/contrib_ref.device_order fed with the
features expecto_variant_reduce_lut stores (outputs inside pattern-filled buffers), and the
predict_by_cluster CLI against the reference's outputs (tests/golden/make_golden_contribs.py)."""
import os

import numpy as np
import pandas as pd
import pytest

import contrib_ref
from conftest import GOLDEN
from guarded import Guarded, P, ST, assert_bits, dev

pytestmark = pytest.mark.gpu
PBC = os.path.join(GOLDEN, "predict_by_cluster")
FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
OUTPUTS = ("contrib", "total", "prop", "clu", "clu_prop")
SHIFTS = {1: [0], 3: [0, -200, 200], 9: [0, -200, -400, -600, -800, 200, 400, 600, 800]}


def no_tf_keep():
    df = pd.read_csv(FEATURES_TSV, sep="\t", index_col=0)
    return np.nonzero((df["Assay type"] != "TF").to_numpy())[0]


def make_case(seed, n, n_shift, keep, n_models, nfeat=2002, shifts=None):
    """Seeded effects with the variants the issue names: dist 0 (both masks), minus strand, a
    distance past the exp table, and an all-negative pair of rows far upstream (-0.0 sums)."""
    rng = np.random.default_rng(seed)
    keep = np.asarray(keep, np.int32)
    shifts = np.asarray(SHIFTS[n_shift] if shifts is None else shifts, np.int32)
    ref = rng.normal(0, 0.05, (len(shifts), n, nfeat)).astype(np.float32)
    alt = (ref + rng.normal(0, 0.01, ref.shape)).astype(np.float32)
    dist = rng.integers(-3000, 3000, n).astype(np.int64)
    strand_plus = (rng.random(n) < 0.5).astype(np.uint8)
    dist[0] = 0
    if n > 1:
        dist[1], strand_plus[1] = 5000, 1               # every d > 0: the upstream weights are all zero
        ref[:, 1], alt[:, 1] = -np.abs(ref[:, 1]), -np.abs(alt[:, 1])
    if n > 2:
        dist[2], strand_plus[2] = 123456, 0             # minus strand, floor(|d|/200) past the table
    w = np.array([float("%g" % x) for x in rng.normal(0.01, 0.02, n_models * 10 * len(keep))]).reshape(n_models, -1)
    return dict(ref=ref, alt=alt, dist=dist, strand_plus=strand_plus, shifts=shifts, keep=keep, w=w, nfeat=nfeat)


def tables(c, lut_len=30):
    """dist, strand, shifts and a decay table of lut_len columns (shorter than the far variant
    needs: that one takes the device exp in both kernels)."""
    fl = np.arange(lut_len, dtype=np.float64)
    lut = np.ascontiguousarray(np.stack([np.exp(-k * fl) for k in (0.01, 0.02, 0.05, 0.1, 0.2)]))
    return dev(c["dist"]), dev(c["strand_plus"]), dev(c["shifts"]), dev(lut)


def features_of(c, tb):
    from expecto_amd.features import variant_reduce
    return [variant_reduce(dev(c[k]), tb).cpu().numpy() for k in ("ref", "alt")]


def call(c, clusters, skip=(), tb=None):
    """The C entry point on guarded outputs; returns {name: host array or None}."""
    from expecto_amd import _lib
    from expecto_amd.features import clusters_csr
    lib = _lib.load()
    tb = tables(c) if tb is None else tb
    d, sp, sh, lut = tb
    S, n, nfeat = c["ref"].shape
    nk, M = len(c["keep"]), c["w"].shape[0]
    n_clu = len(clusters) if clusters else 0
    ptr, mark = clusters_csr(clusters or [], nk)
    ptr_d, mark_d = dev(ptr), dev(np.concatenate([mark, np.zeros(1, np.int32)]))
    shapes = {"contrib": (M, n, nk), "total": (M, n), "prop": (M, n, nk), "clu": (M, n, n_clu), "clu_prop": (M, n, n_clu)}
    out = {k: Guarded(shapes[k], np.float64) for k in OUTPUTS if k not in skip and (n_clu or not k.startswith("clu"))}
    er, ea, keep_d, w_d = dev(c["ref"]), dev(c["alt"]), dev(c["keep"]), dev(c["w"])
    import torch
    status = lib.expecto_variant_contrib(P(er), P(ea), P(d), P(sp), P(sh), S, n, nfeat, P(lut), lut.shape[1], P(keep_d), nk,
                                         P(w_d), M, P(ptr_d) if n_clu else None, P(mark_d) if n_clu else None, n_clu,
                                         *[out[k].ptr if k in out else None for k in OUTPUTS], ST())
    _lib.check(status, "variant_contrib")
    torch.cuda.synchronize()
    return {k: out[k].result() if k in out else None for k in OUTPUTS}


def check(c, clusters, skip=()):
    tb = tables(c)
    fr, fa = features_of(c, tb)
    want = contrib_ref.device_order(fr, fa, c["nfeat"], c["keep"], c["w"], clusters)
    got = call(c, clusters, skip, tb)
    for k in OUTPUTS:
        if k in skip or want[k] is None:
            assert got[k] is None
        else:
            assert_bits(got[k], want[k], k)
    return got, want


def standard_clusters(nk):
    """An empty cluster, one holding every mark, mark 0 in two clusters, a strided one."""
    return [[], list(range(nk)), [0], list(range(0, nk, 3)), [nk - 1, 0]]


@pytest.mark.parametrize("n,n_shift,nk,n_models", [
    (1, 1, 2002, 1), (3, 3, 2002, 3), (65, 9, 2002, 1), (3, 9, 1, 3), (65, 3, 3, 1), (3, 9, "notf", 3), (1, 3, "notf", 1)])
def test_contrib_kernel_bits(n, n_shift, nk, n_models):
    keep = {2002: np.arange(2002), 1: [1234], 3: [5, 700, 2001], "notf": no_tf_keep()}[nk]
    c = make_case(n * 100 + n_shift, n, n_shift, keep, n_models)
    got, want = check(c, standard_clusters(len(keep)))
    if n > 1:       # the all-negative variant: the masked features are -0.0, their differences +0.0
        assert np.isfinite(got["contrib"]).all()


def test_zero_total_gives_numpy_nan_and_inf():
    """Model 0, variant 0: marks 0 and 1 carry the same effects under opposite weights and mark 2
    has alt == ref, so the contributions are c, -c, 0 and the total is exactly 0: prop is
    +-inf, +-inf, nan as numpy's division gives.  Model 1 is all-zero weights: nan everywhere."""
    c = make_case(5, 3, 9, [5, 700, 2001], 2)
    for k in ("ref", "alt"):
        c[k][:, 0, 700] = c[k][:, 0, 5]
    c["alt"][:, 0, 2001] = c["ref"][:, 0, 2001]
    w = c["w"].reshape(2, 10, 3)
    w[0, :, 1] = -w[0, :, 0]
    w[1] = 0.0
    got, want = check(c, [[0, 1, 2], [0], []])
    assert want["total"][0, 0] == 0.0 and np.isinf(got["prop"][0, 0, :2]).all() and np.isnan(got["prop"][0, 0, 2])
    assert np.isnan(got["prop"][1]).all() and np.isnan(got["clu_prop"][1]).all()


def test_no_clusters_and_each_output_null_in_turn():
    c = make_case(6, 3, 3, no_tf_keep(), 3)
    got, _ = check(c, None)
    assert got["clu"] is None and got["clu_prop"] is None
    for name in OUTPUTS:
        check(c, standard_clusters(len(c["keep"])), skip=(name,))
    check(c, standard_clusters(len(c["keep"])), skip=("clu", "clu_prop"))


def test_models_do_not_depend_on_the_batch():
    c = make_case(7, 3, 9, np.arange(2002), 3)
    clusters = standard_clusters(2002)
    all3 = call(c, clusters)
    for m in range(3):
        one = call(dict(c, w=c["w"][m:m + 1].copy()), clusters)
        for k in OUTPUTS:
            assert_bits(one[k][0], all3[k][m], f"{k} of model {m}")


def test_most_shifts_and_marks_beyond_one_tile():
    """819 shifts: the weights alone take 64 KiB of LDS (the opt-in size).  nfeat = 4200: the marks
    go in three tiles of 2048 and every model recomputes a tile's differences."""
    c = make_case(8, 2, 819, [0, 2001], 2, shifts=(np.arange(819) - 409) * 200)
    check(c, [[0, 1], [1]])
    c = make_case(9, 2, 3, np.arange(0, 4200), 2, nfeat=4200)
    check(c, standard_clusters(4200))


def test_limits_are_refused():
    from expecto_amd import _lib
    lib = _lib.load()
    none = [None] * 5
    args = lambda S, n, nk, M, n_clu: (None, None, None, None, None, S, n, 2002, None, 0, None, nk, None, M, None, None,
                                       n_clu, *none, None)
    for a, text in ((args(820, 1, 1, 1, 0), "n_shift <= 819"), (args(9, 65536, 1, 1, 0), "65535 variants"),
                    (args(9, 1, 0, 1, 0), "nk"), (args(9, 1, 2003, 1, 0), "nk"), (args(9, 1, 1, 0, 0), "n_models")):
        assert lib.expecto_variant_contrib(*a) == -1
        assert text in lib.expecto_last_error().decode()
    assert lib.expecto_variant_contrib(*args(9, 0, 1, 1, 0)) == 0
    x = dev(np.zeros(8, np.float64))
    big = (None, None, None, None, None, 819, 1, 20000, None, 0, None, 14000, None, 1, None, None, 0, *none, None)
    assert lib.expecto_variant_contrib(*big) == -1      # null pointers are looked at first
    assert "null" in lib.expecto_last_error().decode()
    # 8 * (8190 + 14000 + 2) bytes > 160 KiB: refused before any launch
    big = (P(x), P(x), P(x), P(x), P(x), 819, 1, 20000, None, 0, P(x), 14000, P(x), 1, None, None, 0, *none, None)
    assert lib.expecto_variant_contrib(*big) == -1 and "LDS" in lib.expecto_last_error().decode()


def test_python_api_chunks_past_65535_variants():
    import torch
    from expecto_amd.features import variant_contributions, variant_features
    rng = np.random.default_rng(10)
    n, F = 65537, 4
    ref = rng.normal(0, 0.05, (1, n, F)).astype(np.float32)
    alt = (ref + rng.normal(0, 0.01, ref.shape)).astype(np.float32)
    dist, sp = rng.integers(-2000, 2000, n), rng.random(n) < 0.5
    w = rng.normal(0.01, 0.02, (2, 20))
    res = variant_contributions(dev(ref), dev(alt), dist, sp, [0], [1, 3], w, clusters=[[0, 1], [1]])
    fr, fa = (variant_features(dev(x), dist, sp, [0]).cpu().numpy() for x in (ref, alt))
    want = contrib_ref.device_order(fr, fa, F, [1, 3], w, [[0, 1], [1]])
    for k in OUTPUTS:
        assert_bits(getattr(res, k).cpu().numpy(), want[k], k)
    with pytest.raises(RuntimeError, match="ascending"):
        variant_contributions(dev(ref), dev(alt), dist, sp, [0], [3, 1], w)
    # only the outputs asked for are allocated and written
    some = variant_contributions(dev(ref), dev(alt), dist, sp, [0], [1, 3], w, clusters=[[0, 1], [1]],
                                 outputs=("prop", "clu_prop"))
    assert some.contrib is None and some.total is None and some.clu is None
    for k in ("prop", "clu_prop"):
        assert_bits(getattr(some, k).cpu().numpy(), want[k], k)
    with pytest.raises(RuntimeError, match="outputs"):
        variant_contributions(dev(ref), dev(alt), dist, sp, [0], [1, 3], w, outputs=("props",))
    assert torch.cuda.is_available()


# ---- the CLI on the golden fixtures -----------------------------------------------------------
def _write_inputs(d):
    from expecto_amd import h5
    chrom = np.load(os.path.join(GOLDEN, "chromatin.npz"))
    feats = np.load(os.path.join(GOLDEN, "predict_features.npz"))
    os.makedirs(d / "out", exist_ok=True)
    for s in (0, -200, 200):
        h5.write(str(d / "out" / f"snps.shift_{s}.diff.h5"), {k: chrom[f"{k}_{s}"] for k in ("diff", "ref", "alt")})
    (d / "coor.vcf").write_text("##fileformat=VCFv4.3\n" + "".join(str(r) + "\n" for r in feats["coor_rows"]))
    (d / "genes.tsv").write_text("".join(str(r) + "\n" for r in feats["gene_rows"]))
    return ["--belugaFeatures", FEATURES_TSV, "--coorFile_chromatin", str(d / "coor.vcf"), "--geneFile",
            str(d / "genes.tsv"), "--snpEffectFilePattern", str(d / "out" / "snps.shift_SHIFT.diff.h5"),
            "--maxshift", "200", "--batchSize", "3", "--intersect_with_lambert"]


def _read(path):
    return pd.read_csv(path, sep="\t", float_precision="round_trip")


@pytest.fixture(scope="module")
def golden_case():
    return contrib_ref.golden_inputs(GOLDEN)


def _check_sed_columns(got, want, name):
    assert list(got["index"]) == list(want["index"]), f"{name}: row order"
    base = [c for c in want.columns[:13] if c in ("REF", "ALT", "SED") or c.startswith("SED_")]
    other = [c for c in want.columns[:13] if c not in base]
    assert got[other].astype(str).equals(want[other].astype(str)), name
    # The golden's printed digits round-trip to its float64 values.  The device features are bitwise
    # the reference's (exp table from numpy, products and sums in its order) and the scoring kernel is
    # bitwise the restated gblinear (tests/test_gpu_predict.py), so the scores are equal, not close.
    for col in base:
        assert np.array_equal(got[col].to_numpy(), want[col].to_numpy()), (name, col)


def test_cli_rsat_mode_matches_the_reference(tmp_path, capsys, monkeypatch, golden_case):
    from expecto_amd import predict_by_cluster as pbc
    common = _write_inputs(tmp_path)
    monkeypatch.chdir(PBC)              # ./resources/*.csv
    out = tmp_path / "pout"
    pbc.main(["--model_save_file", os.path.join(PBC, "model.save"), *common,
              "--rsat_clusters_tab", os.path.join(PBC, "clusters_motif_names.tab"), "-o", str(out)])
    assert capsys.readouterr().out == open(os.path.join(PBC, "stdout.txt")).read()
    assert open(out / "rsat_clusters.tsv").read() == open(os.path.join(PBC, "rsat_clusters.tsv")).read()
    assert not os.path.exists(out / "sed.tsv")
    g = golden_case
    r = contrib_ref.reference_order(g["weights"], g["ref"], g["alt"], g["assay_clusters"])
    members = [[f for f, ids in enumerate(g["assay_clusters"]) if cid in ids] for cid in r["columns"]]
    b = contrib_ref.bounds(g["weights"], g["ref"], g["alt"], r, members)
    assert b["prop_rows"].all() and b["clu_rows"].all()
    for name in ("sed.csv", "sed_sorted_by_magnitude.tsv", "sed_sorted_by_proportion.tsv",
                 "sed_sorted_by_proportion_with_contribs.tsv", "cluster_contribs.tsv"):
        got, want = _read(out / name), _read(os.path.join(PBC, name))
        assert open(out / name).readline() == open(os.path.join(PBC, name)).readline(), f"{name}: header"
        _check_sed_columns(got, want, name)
        extra = want.shape[1] - 13
        if name.endswith("contribs.tsv"):
            bound = b["prop" if extra == 40 else "clu_prop"][want["index"].to_numpy()]
            err = np.abs(got.iloc[:, 13:].to_numpy() - want.iloc[:, 13:].to_numpy())
            assert extra in (40, 4) and np.all(err <= bound), (name, float((err / bound).max()))


def test_cli_feature_clusters_mode_and_two_models(tmp_path, capsys, monkeypatch, golden_case):
    """--feature_clusters_df against reference_order (the reference script itself calls pd.match,
    which pandas no longer has); two models in one run write what each writes alone."""
    from expecto_amd import predict_by_cluster as pbc
    from expecto_amd.xgblinear import GBLinear
    common = _write_inputs(tmp_path)
    monkeypatch.chdir(PBC)
    g = golden_case
    labels = pd.Series(np.arange(40) % 3 * 2)                  # labels 0, 2, 4 -> cluster_0..2
    pd.DataFrame({"cluster": np.repeat(labels.to_numpy(), 10)}).to_csv(tmp_path / "all_feature_clusters.tsv", sep="\t")
    m = GBLinear.load(os.path.join(PBC, "model.save"))
    second = GBLinear(-m.weights[::-1].copy() * 0.5, m.bias.copy(), m.base_score)
    second.save_legacy(str(tmp_path / "second.save"))
    files = [os.path.join(PBC, "model.save"), str(tmp_path / "second.save")]
    fc = ["--feature_clusters_df", str(tmp_path / "all_feature_clusters.tsv")]
    pbc.main(["--model_save_file", *files, *common, *fc, "-o", str(tmp_path / "both")])
    # predict_by_cluster.py prints the mask messages in every batch and once at line 298, not ahead
    lines = sum([[f"Processing {i}th batch of 3", "intersecting with Lambert data",
                  "Number of features included in model: 40"] for i in range(3)], [])
    lines += ["intersecting with Lambert data", "Number of features included in model: 40"]
    assert capsys.readouterr().out == "".join(x + "\n" for x in lines)
    for i, f in enumerate(files):
        pbc.main(["--model_save_file", f, *common, *fc, "-o", str(tmp_path / f"one{i}")])
        assert capsys.readouterr().out == "".join(x + "\n" for x in lines)
    names = ("sed.csv", "sed_sorted_by_magnitude.csv", "sed_sorted_by_proportion.csv",
             "sed_sorted_by_proportion_with_contribs.csv", "cluster_contribs.csv")
    for i, stem in enumerate(("model", "second")):
        for name in names:
            assert open(tmp_path / "both" / stem / name).read() == open(tmp_path / f"one{i}" / name).read(), (stem, name)
    assert not os.path.exists(tmp_path / "one0" / "rsat_clusters.tsv")
    for name in names[:3]:              # model.save is the golden run's model: the same scores, digit for digit
        gold = name if name == "sed.csv" else name.replace(".csv", ".tsv")
        _check_sed_columns(_read(tmp_path / "one0" / name), _read(os.path.join(PBC, gold)), name)
    from oracle import gblinear_np
    for i, model in enumerate((m, second)):
        sed = _read(tmp_path / f"one{i}" / "sed.csv")
        want = {k: gblinear_np.predict(g[k.lower()], model.weights[:, 0], model.bias[0], model.base_score)
                .astype(np.float64) for k in ("REF", "ALT")}
        want["SED"] = want["ALT"] - want["REF"]
        for k in ("REF", "ALT", "SED"):
            assert np.array_equal(sed[k].to_numpy(), want[k]), (i, k)
        w = model.dump_weights()
        r = contrib_ref.reference_order(w, g["ref"], g["alt"], labels)
        members = [np.nonzero(labels.to_numpy() == c)[0].tolist() for c in (0, 2, 4)]
        b = contrib_ref.bounds(w, g["ref"], g["alt"], r, members)
        assert b["prop_rows"].all() and b["clu_rows"].all()
        got = _read(tmp_path / f"one{i}" / "cluster_contribs.csv")
        assert list(got.columns[13:]) == ["cluster_0", "cluster_1", "cluster_2"]
        order = got["index"].to_numpy()
        assert np.all(np.abs(got.iloc[:, 13:].to_numpy() - r["clu_prop"][order]) <= b["clu_prop"][order])
        got = _read(tmp_path / f"one{i}" / "sed_sorted_by_proportion_with_contribs.csv")
        header = open(tmp_path / f"one{i}" / "sed_sorted_by_proportion_with_contribs.csv").readline().rstrip("\n")
        assert header.split("\t")[13:] == g["features"]["Assay type + assay + cell type"].to_numpy()[g["keep"]].tolist()
        assert np.all(np.abs(got.iloc[:, 13:].to_numpy() - r["prop"][got["index"].to_numpy()]) <= b["prop"][order])
