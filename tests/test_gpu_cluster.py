"""Ward clustering on the device: the pairwise-distance kernel of cluster.hip through its C entry
point, ``interpret_features.ward_tree`` and the ``python -m expecto_amd.interpret_features`` CLI.

The kernel computes one 64 x 64 tile of pairs per workgroup (TILE = 64 points per panel) and stages
the panels through LDS 32 dimensions at a time (STAGE = 32); the shapes below sit on both sides of
both.  Outputs lie in pattern-filled buffers (tests/guarded.py) and inputs in NaN-filled ones with
``ld > d``, so a store outside the condensed matrix or a load from the padding fails the test.
Every comparison with the restatement (tests/ward_ref.py) is bitwise."""
import functools
import io
import os

import numpy as np
import pandas as pd
import pytest
import torch

import ward_ref
from conftest import GOLDEN
from guarded import Guarded, ST, assert_bits

pytestmark = pytest.mark.gpu

TILE, STAGE = 64, 32
FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
GOLD = os.path.join(GOLDEN, "interpret_features")


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


class Padded:
    """X [n, d] float64 on the device with row stride ld > d inside NaN: the padding of every row and
    ``margin`` doubles before the first and after the last row are NaN."""

    def __init__(self, X, ld, margin=64):
        n, d = X.shape
        assert ld > d
        host = np.full(margin + n * ld + margin, np.nan)
        host[margin:margin + n * ld].reshape(n, ld)[:, :d] = X
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin


def device_pdist(lib, X, ld=None):
    n, d = X.shape
    x = Padded(X, ld if ld is not None else d + 3)
    out = Guarded((max(n * (n - 1) // 2, 0),), np.float64)
    st = lib.expecto_pairwise_euclidean(x.ptr, n, d, ld if ld is not None else d + 3, out.ptr, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    return out.result()


EDGE_SHAPES = [(2, 1), (17, 7), (65, 257), (130, 1031),
               (TILE + 1, STAGE - 1), (TILE + 1, STAGE + 1), (2 * TILE - 1, STAGE - 1), (2 * TILE - 1, STAGE + 1)]


@pytest.mark.parametrize("n,d", EDGE_SHAPES)
def test_kernel_edges(lib, n, d):
    """n and d off the tile and the stage: one pair; less than a tile; one tile + 1 (a second tile row of
    one point: two diagonal tiles and a one-column tile); two tiles - 1; three tile rows (130); d of one
    stage -1 / +1 and of many stages plus a tail (257 = 8 x 32 + 1, 1031 = 32 x 32 + 7).  Signed values."""
    X = np.random.default_rng([n, d]).normal(size=(n, d)) * np.random.default_rng([d, n]).gamma(0.7, 2.0, (1, d))
    assert_bits(device_pdist(lib, X), ward_ref.pdist(X), f"pdist {n}x{d}")


def test_kernel_nothing_to_do(lib):
    """n = 1 (and 0) writes nothing; d = 0 writes +0.0 for every pair."""
    for n in (0, 1):
        out = Guarded((4,), np.float64)
        x = Padded(np.ones((max(n, 1), 4)), 6)
        assert lib.expecto_pairwise_euclidean(x.ptr, n, 4, 6, out.ptr, ST()) == 0
        torch.cuda.synchronize()
        assert out.untouched()
    got = device_pdist(lib, np.empty((3, 0)), ld=2)
    assert_bits(got, np.zeros(3), "d = 0")
    assert_bits(got, ward_ref.pdist(np.empty((3, 0))), "d = 0 vs restatement")


def test_kernel_refusals(lib):
    out = Guarded((4,), np.float64)
    x = Padded(np.ones((3, 4)), 6)
    for args, text in (((x.ptr, -1, 4, 6, out.ptr), "negative shape"), ((x.ptr, 3, 4, 3, out.ptr), "ld < d"),
                       ((None, 3, 4, 6, out.ptr), "null argument"), ((x.ptr, 3, 4, 6, None), "null argument"),
                       ((x.ptr, (1 << 21) + 1, 4, 6, out.ptr), "at most 2097152 points")):
        assert lib.expecto_pairwise_euclidean(*args, ST()) == -1
        assert text in lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    assert out.untouched()


def test_kernel_input_values(lib):
    """Signed zeros, denormals, two identical rows (+0.0 exactly), squares that underflow, and values
    near 1e150 whose squared differences overflow: inf out, as the restatement's."""
    rng = np.random.default_rng(77)
    n, d = 21, 37
    X = rng.normal(size=(n, d))
    X[0, :9], X[1, :9] = -0.0, 0.0
    X[2] = 5e-324 * rng.integers(-40, 40, d)
    X[3] = X[2]
    X[4] = 1e-310 * rng.normal(size=d)
    X[5], X[6] = 1e-170 * rng.normal(size=d), -1e-160 * rng.normal(size=d)
    X[7, 3], X[8, 3], X[9, 30] = 1e150, -1.3e150, 2e154     # squares 1e300 (finite) and 4e308 (inf)
    X[10] = X[0]
    X[10, 20:] = -X[10, 20:]
    want = ward_ref.pdist(X)
    got = device_pdist(lib, X)
    assert_bits(got, want, "special values")
    at = lambda i, j: got[ward_ref.condensed_index(n, i, j)]
    assert at(2, 3) == 0.0 and not np.signbit(at(2, 3))
    assert at(2, 4) == 0.0 and 0 < at(5, 6) < 1e-150        # squares below the denormals; denormal squares
    assert 2e150 < at(7, 8) < 3e150
    assert np.isinf(at(0, 9)) and np.isinf(got).sum() == n - 1 and not np.isnan(got).any()


@functools.lru_cache(maxsize=None)
def tree_case(name):
    X = ward_ref.gamma_points(130, 257) if name == "gamma" else ward_ref.tie_points(64, 6)
    X.setflags(write=False)
    return X, ward_ref.ward(X)


@pytest.mark.parametrize("name", ["gamma", "ties"])
def test_ward_tree(name):
    from expecto_amd.interpret_features import ward_tree
    X, (children, heights, _) = tree_case(name)
    for arg in (X, torch.from_numpy(X.copy()).cuda()):
        got_c, got_h = ward_tree(arg)
        assert got_c.dtype == np.int64 and got_h.dtype == np.float64
        assert_bits(got_c, children, name + " children")
        assert_bits(got_h, heights, name + " heights")
    # a strided view of a wider matrix is made contiguous on the device
    wide = torch.full((X.shape[0], X.shape[1] + 5), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 2:2 + X.shape[1]] = torch.from_numpy(X.copy()).cuda()
    got_c, got_h = ward_tree(wide[:, 2:2 + X.shape[1]])
    assert_bits(got_c, children, name + " children, strided")
    assert_bits(got_h, heights, name + " heights, strided")


@pytest.mark.parametrize("name", ["gamma", "ties"])
def test_ward_tree_equals_sklearn(name):
    pytest.importorskip("scipy")
    pytest.importorskip("sklearn")
    from sklearn.cluster import AgglomerativeClustering
    from expecto_amd.interpret_features import ward_tree
    X, _ = tree_case(name)
    model = AgglomerativeClustering(distance_threshold=0, n_clusters=None).fit(X)
    got_c, got_h = ward_tree(X)
    assert np.array_equal(got_c, model.children_)
    assert_bits(got_h, model.distances_, name + " distances_")


# ---- CLI -------------------------------------------------------------------------------------

def run_cli(capsys, argv):
    from expecto_amd import interpret_features
    capsys.readouterr()
    interpret_features.main([str(a) for a in argv])
    return capsys.readouterr().out


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_grouped_golden(tmp_path, capsys):
    """The reference interpret_features_grouped.py's files and stdout on the regenerated golden input
    (2002 marks x 22 training genes x 10), byte for byte."""
    x_path, anno_path, exp_path = ward_ref.write_interpret_inputs(str(tmp_path))
    for p in (anno_path, exp_path):     # the committed CSVs are the generator's
        assert read(p) == read(os.path.join(GOLD, os.path.basename(p)))
    out_dir = tmp_path / "iout"
    stdout = run_cli(capsys, ["--grouped", "--belugaFeatures", FEATURES_TSV, "--targetIndex", 1, "--expFile", exp_path,
                              "--inputFile", x_path, "--annoFile", anno_path, "--pseudocount", 0, "--out_dir", out_dir])
    assert stdout.encode() == read(os.path.join(GOLD, "stdout.txt"))
    for t in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
        assert read(out_dir / t) == read(os.path.join(GOLD, t)), t
    labels = pd.read_csv(out_dir / "all_feature_clusters.tsv", sep="\t", index_col=0)["cluster"].to_numpy()
    for i in (0, 57, 109):
        part = pd.read_csv(out_dir / "clusters" / f"cluster_{i}.tsv", sep="\t", index_col=0)
        assert np.array_equal(part.index.to_numpy(), np.nonzero(labels == i)[0] + 1)
    z = np.load(out_dir / "clustering.npz")
    assert int(z["n_leaves"]) == 2002 and z["children"].shape == (2001, 2) and z["distances"].shape == (2001,)


N_MARKS_SMALL = 23


def small_inputs(root, kind):
    """23 marks, 30 genes.  kind "generic": decay block k scaled by 0.8^k with noise, no structure by
    mark; "by_mark": four well separated families of marks whose ten columns are near copies."""
    rng = np.random.default_rng({"generic": 301, "by_mark": 302}[kind])
    n_genes, m = 30, N_MARKS_SMALL
    if kind == "generic":
        X = np.concatenate([rng.gamma(0.7, 2.0, (n_genes, m)) * 0.8 ** k for k in range(10)], axis=1)
    else:
        centre = rng.gamma(2.0, 10.0, (4, n_genes))
        X = np.concatenate([centre[np.arange(m) % 4].T + 0.01 * rng.normal(size=(n_genes, m)) for _ in range(10)],
                           axis=1)
    os.makedirs(root, exist_ok=True)
    paths = {k: os.path.join(root, v) for k, v in (("x", "X.npy"), ("anno", "anno.csv"), ("exp", "exp.csv"),
                                                   ("feat", "features.tsv"))}
    np.save(paths["x"], X)
    chrom = ["chr1", "chr3", "chr8", "chr17", "chrX"]
    types = ["protein_coding", "lincRNA", "protein_coding"]
    with open(paths["anno"], "w") as f:
        f.write("id,symbol,seqnames,strand,TSS,CAGE_representative_TSS,type\n")
        for g in range(n_genes):
            f.write(f"ENSG{g:04d},G{g},{chrom[g % 5]},+,{100 * g},{100 * g},{types[g % 3]}\n")
    with open(paths["exp"], "w") as f:
        f.write("a,b\n" + "".join(f"{1.5 + g},{0.25 * g}\n" for g in range(n_genes)))
    with open(FEATURES_TSV) as src, open(paths["feat"], "w") as f:
        f.writelines(src.readlines()[:1 + m])
    anno = pd.read_csv(paths["anno"])
    train = ~anno["seqnames"].isin(["chrX", "chrY", "chr8"]).to_numpy() & (anno["type"] == "protein_coding").to_numpy()
    train[0] = False        # exp column b is 0 for gene 0: log(0 + 0) is not finite
    return paths, X[train]


def small_argv(paths, out_dir, *extra):
    return ["--belugaFeatures", paths["feat"], "--targetIndex", 1, "--expFile", paths["exp"], "--inputFile", paths["x"],
            "--annoFile", paths["anno"], "--filterStr", "pc", "--pseudocount", 0, "--out_dir", out_dir, *extra]


def test_cli_ungrouped(tmp_path, capsys):
    """230 points (23 marks x 10 decay columns) over the protein-coding training genes: labels equal
    the restatement's (and sklearn's), laid out as interpret_features.py:121-127; the file of this
    structureless input is refused by predict_by_cluster.feature_clusters (a mark's ten rows differ)."""
    from expecto_amd import predict_by_cluster
    paths, X_train = small_inputs(str(tmp_path / "in"), "generic")
    assert X_train.shape == (11, 230)     # 30 genes less chr8 / chrX, lincRNA and the zero expression value
    out_dir = tmp_path / "out"
    stdout = run_cli(capsys, small_argv(paths, out_dir))
    assert stdout == "Cell type: b\nClustering complete tree and caching...\n"
    children, heights, _ = ward_ref.ward(X_train.T)
    z = np.load(out_dir / "clustering.npz")
    assert_bits(z["children"], children, "children")
    assert_bits(z["distances"], heights, "distances")
    labels = ward_ref.cut(children, 230, 10)
    try:
        from sklearn.cluster import AgglomerativeClustering
    except ImportError:
        pass
    else:
        assert np.array_equal(AgglomerativeClustering(n_clusters=10).fit(X_train.T).labels_, labels)
    df = pd.read_csv(out_dir / "all_feature_clusters.tsv", sep="\t", index_col=0)
    feats = pd.read_csv(paths["feat"], sep="\t", index_col=0)
    assert len(df) == 230 and list(df.columns[-2:]) == ["coeff_idx", "cluster"]
    assert np.array_equal(df.index.to_numpy(), np.arange(230))
    assert np.array_equal(df["coeff_idx"].to_numpy(), np.tile(np.arange(10), N_MARKS_SMALL))
    assert np.array_equal(df["cluster"].to_numpy(), labels.reshape(10, N_MARKS_SMALL).T.ravel())   # row 10 f + k: point k*23 + f
    assert list(df["Cell type"]) == list(np.repeat(feats["Cell type"].to_numpy(), 10))
    assert set(os.listdir(out_dir / "clusters")) == {f"cluster_{i}.tsv" for i in range(10)}
    assert not (out_dir / "cluster_sizes.tsv").exists()
    part = pd.read_csv(out_dir / "clusters" / "cluster_3.tsv", sep="\t", index_col=0)
    assert np.array_equal(part.index.to_numpy(), np.nonzero(df["cluster"].to_numpy() == 3)[0])
    per_mark = df["cluster"].to_numpy().reshape(N_MARKS_SMALL, 10)
    assert (per_mark != per_mark[:, :1]).any()
    with pytest.raises(ValueError, match="carry different labels"):
        predict_by_cluster.feature_clusters(str(out_dir / "all_feature_clusters.tsv"), N_MARKS_SMALL)


def test_cli_ungrouped_accepted_by_predict_by_cluster(tmp_path, capsys):
    """Marks in four separated families, ten near-equal columns each, cut into 4: every mark's ten
    labels agree and predict_by_cluster.feature_clusters returns the families."""
    from expecto_amd import predict_by_cluster
    paths, X_train = small_inputs(str(tmp_path / "in"), "by_mark")
    out_dir = tmp_path / "out"
    run_cli(capsys, small_argv(paths, out_dir, "--n_clusters", 4, "--clustering_with_distances"))
    labels = ward_ref.cut(ward_ref.ward(X_train.T)[0], 230, 4).reshape(10, N_MARKS_SMALL).T
    assert (labels == labels[:, :1]).all()
    ids, members = predict_by_cluster.feature_clusters(str(out_dir / "all_feature_clusters.tsv"), N_MARKS_SMALL)
    assert ids == [0, 1, 2, 3]
    assert members == [np.nonzero(labels[:, 0] == c)[0].tolist() for c in range(4)]
    assert sorted(map(tuple, members)) == sorted(tuple(range(r, N_MARKS_SMALL, 4)) for r in range(4))
    with pytest.raises(ValueError, match="rows for 22 kept marks"):
        predict_by_cluster.feature_clusters(str(out_dir / "all_feature_clusters.tsv"), N_MARKS_SMALL - 1)


def test_cli_round_trip(tmp_path, capsys, monkeypatch):
    """--clustering_joblib <out>/clustering.npz with another --n_clusters writes what a fresh run with
    that count writes, and never reaches the device."""
    from expecto_amd import interpret_features
    paths, _ = small_inputs(str(tmp_path / "in"), "generic")
    first, fresh, again = (tmp_path / d for d in ("first", "fresh", "again"))
    run_cli(capsys, small_argv(paths, first, "--grouped", "--n_clusters", 5))
    run_cli(capsys, small_argv(paths, fresh, "--grouped", "--n_clusters", 9))

    def no_device(*a, **k):
        raise AssertionError("the tree was recomputed")
    monkeypatch.setattr(interpret_features, "ward_tree", no_device)
    stdout = run_cli(capsys, small_argv(paths, again, "--grouped", "--n_clusters", 9, "--clustering_joblib",
                                        first / "clustering.npz"))
    assert stdout == f"Cell type: b\nLoading clustering model from {first / 'clustering.npz'}...\n"
    for t in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
        assert read(again / t) == read(fresh / t), t
    assert read(first / "all_feature_clusters.tsv") != read(fresh / "all_feature_clusters.tsv")
    assert not (again / "clustering.npz").exists()
    with pytest.raises(ValueError, match="23 leaves"):      # a grouped tree cannot label the 230 features
        run_cli(capsys, small_argv(paths, tmp_path / "bad", "--clustering_joblib", first / "clustering.npz"))
