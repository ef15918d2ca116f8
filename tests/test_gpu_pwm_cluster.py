"""``expecto_pwm_compare`` on the device (csrc/motif_cluster.hip), through its C entry point,
``expecto_amd.cluster_by_pwm`` and its command line.

Outputs lie in pattern-filled buffers (tests/guarded.py) and the frequencies inside NaN margins, so a
store outside an output or a load outside the motifs fails the test.  Every comparison with the
restatement (tests/pwm_cluster_ref.py) is bitwise for the float arrays and exact for the int arrays.
The kernel takes a 16 x 16 tile of motif pairs per workgroup."""
import functools
import os

import numpy as np
import pytest
import torch

import pwm_cluster_ref as ref
from guarded import Guarded, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

T = 16                                                # the kernel's tile edge
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_by_pwm")
NAMES = ("cor", "ncor", "dist", "offset", "strand", "width")
PLANTED_SEED = 2                                      # see test_cluster_end_to_end


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cbp():
    from expecto_amd import cluster_by_pwm
    return cluster_by_pwm


@functools.lru_cache(maxsize=None)
def motif_set(kind, M):
    """Count matrices, shared and read-only."""
    rng = np.random.default_rng([M, len(kind)])
    if kind == "random":
        widths = rng.integers(4, 26, M)
    elif kind == "w1":
        widths = [1] * M
    elif kind == "w64":
        widths = [64] * M
    else:                                             # min_w - 1, min_w and 64 side by side in one tile
        widths = [(4, 5, 64)[k % 3] for k in range(M)]
    mats = tuple(ref.random_counts(int(w), 100 * M + k) for k, w in enumerate(widths))
    for m in mats:
        m.setflags(write=False)
    return mats


@functools.lru_cache(maxsize=None)
def reference(kind, M, min_w=5, pseudo=1.0):
    out = ref.compare(motif_set(kind, M), min_w, pseudo)
    for a in out:
        a.setflags(write=False)
    return out


def pack(mats, pseudo=1.0):
    """(freq float64 [total, 4], col_ptr int32).  The kernel centres f itself: it is handed f, checked here
    to centre to the restatement's bits."""
    c = np.concatenate([np.asarray(m, np.float64) for m in mats]) if mats else np.zeros((0, 4))
    freq = (c + pseudo / 4) / ((((c[:, 0] + c[:, 1]) + c[:, 2]) + c[:, 3]) + pseudo)[:, None]
    want = np.array(sum((ref.frequencies(m, pseudo) for m in mats), []), np.float64)
    assert np.array_equal((freq - 0.25).ravel().view(np.uint64), want.view(np.uint64))
    col_ptr = np.zeros(len(mats) + 1, np.int32)
    col_ptr[1:] = np.cumsum([np.asarray(m).shape[0] for m in mats])
    return np.ascontiguousarray(freq), col_ptr


class Freq:
    """float64 [total, 4] on the device between margins of NaN."""

    def __init__(self, freq, margin=1024):
        host = np.full(2 * margin + freq.size, np.nan, np.float64)
        host[margin:margin + freq.size] = freq.ravel()
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin


def compare_device(lib, mats, min_w=5, pseudo=1.0, status=0, col_ptr_edit=None):
    """The entry point on guarded outputs -> the six arrays, None when nothing may be written, or the
    message of the refusal expected."""
    freq, col_ptr = pack(mats, pseudo)
    if col_ptr_edit is not None:
        col_ptr = col_ptr_edit(col_ptr)
    M = len(col_ptr) - 1
    npair = M * (M - 1) // 2
    src, d_ptr = Freq(freq), dev(col_ptr)
    outs = [Guarded((max(1, npair),), np.float64, offset=8 * k) for k in range(3)]
    outs += [Guarded((max(1, npair),), np.int32, offset=4 * k) for k in range(3)]
    st = lib.expecto_pwm_compare(src.ptr, col_ptr.ctypes.data, d_ptr.data_ptr(), M, min_w, *[o.ptr for o in outs], ST())
    torch.cuda.synchronize()
    if status != 0:
        assert st == status
        assert all(o.untouched() for o in outs)
        return lib.expecto_last_error().decode()
    assert st == 0, lib.expecto_last_error().decode()
    if npair == 0:
        assert all(o.untouched() for o in outs)
        return None
    return tuple(o.result() for o in outs)


def assert_compare(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert_bits(g, w, f"{what}: {name}")
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any() and (got[2] >= 0).all()


# ---- expecto_pwm_compare -------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_motif_counts_around_the_tile(lib, M):
    got = compare_device(lib, motif_set("random", M))
    if M == 1:
        assert got is None
        return
    assert_compare(got, reference("random", M), f"M={M}")


@pytest.mark.parametrize("kind", ["w1", "w64", "mixed"])
def test_width_sets(lib, kind):
    """All 1 (a single alignment per strand), all 64 (16 of them fill a group's LDS to its largest) and
    min_w - 1, min_w, 64 in one tile."""
    M = T + 1
    want = reference(kind, M)
    assert_compare(compare_device(lib, motif_set(kind, M)), want, kind)
    if kind == "w1":
        assert (want[3] == 0).all() and (want[5] == 1).all()
    if kind == "mixed":
        assert {4, 5}.issubset(set(want[5].tolist())) and want[5].max() > 5


@pytest.mark.parametrize("min_w", [1, 64])
def test_min_w(lib, min_w):
    """min_w = 1 admits overlaps of one column; min_w = 64 leaves the shorter motif inside the longer."""
    M = T + 1
    want = reference("mixed", M, min_w)
    assert_compare(compare_device(lib, motif_set("mixed", M), min_w=min_w), want, f"min_w={min_w}")
    widths = [m.shape[0] for m in motif_set("mixed", M)]
    shorter = np.array([min(widths[i], widths[j]) for i in range(M) for j in range(i + 1, M)])
    if min_w == 64:
        assert (want[5] == shorter).all()
    else:
        assert (want[5] < shorter).any()


def special_set():
    """0 P, 1 a copy of P, 2 Q, 3 Q's reverse complement, 4 a palindrome, 5 its copy, 6 all-uniform columns,
    7 A, 8 B whose last five columns are A's first five, 9 C whose first five columns are A's last five."""
    P, Q, A = ref.random_counts(9, 1), ref.random_counts(11, 2), ref.random_counts(8, 3, sites=400)
    half = ref.random_counts(4, 4)
    pal = np.concatenate([half, ref.rc_counts(half)])
    uniform = np.full((7, 4), 5.0)
    B = np.concatenate([ref.random_counts(3, 5, sites=400), A[:5]])
    C = np.concatenate([A[3:], ref.random_counts(3, 6, sites=400)])
    return [P, P.copy(), Q, ref.rc_counts(Q), pal, pal.copy(), uniform, A, B, C]


@pytest.mark.parametrize("pseudo", [0.0, 1.0])
def test_special_motifs(lib, pseudo):
    mats = special_set()
    M = len(mats)
    want = ref.compare(mats, 5, pseudo)
    at = lambda i, j: ref.condensed_index(M, i, j)
    cor, ncor, dist, offset, strand, width = want
    # the restatement itself shows the cases to be what they are meant to be
    assert abs(ncor[at(0, 1)] - 1.0) < 1e-12 and strand[at(0, 1)] == 0 and offset[at(0, 1)] == 0 and width[at(0, 1)] == 9
    assert strand[at(2, 3)] == 1 and offset[at(2, 3)] == 0 and abs(ncor[at(2, 3)] - 1.0) < 1e-12
    assert all(strand[at(i, 4)] == 0 for i in range(4)) and strand[at(4, 5)] == 0      # D before R at equal Ncor
    assert ncor[at(4, 5)] > 0.99
    assert offset[at(7, 8)] == -3 and offset[at(7, 9)] == 3 and strand[at(7, 8)] == 0 and strand[at(7, 9)] == 0
    assert width[at(7, 8)] == 5 and width[at(7, 9)] == 5
    if pseudo == 0.0:
        for k in range(M):
            if k != 6:
                p = at(min(k, 6), max(k, 6))
                assert cor[p] == 0.0 and ncor[p] == 0.0 and dist[p] == 1.0 and strand[p] == 0
                assert offset[p] == -(mats[max(k, 6)].shape[0] - 5)                    # the first alignment
    got = compare_device(lib, mats, pseudo=pseudo)
    assert_compare(got, want, f"special pseudo={pseudo}")


def test_refusals_and_empty_calls(lib):
    ok = ref.random_counts(5, 1)
    assert "width 65" in compare_device(lib, [ok, np.concatenate([ref.random_counts(64, 1), ok[:1]]), ok], status=-1)
    assert "width 0" in compare_device(lib, [ok, ok[:0], ok], status=-1)
    assert "min_w" in compare_device(lib, [ok, ok], min_w=0, status=-1)

    def decrease(col_ptr):
        col_ptr = col_ptr.copy()
        col_ptr[2] = 3
        return col_ptr
    assert "decreasing" in compare_device(lib, [ok, ok, ok], col_ptr_edit=decrease, status=-1)
    assert compare_device(lib, [ok]) is None
    assert lib.expecto_pwm_compare(None, None, None, 4097, 5, None, None, None, None, None, None, ST()) == -1
    assert "4097 motifs" in lib.expecto_last_error().decode()
    col_ptr = np.array([0, 3, 6], np.int32)
    assert lib.expecto_pwm_compare(None, col_ptr.ctypes.data, None, 2, 5, None, None, None, None, None, None, ST()) == -1
    assert "null" in lib.expecto_last_error().decode()
    assert lib.expecto_pwm_compare(None, None, None, 0, 5, None, None, None, None, None, None, ST()) == 0


# ---- Python ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planted_reference():
    mats, names, fam = ref.planted(PLANTED_SEED)
    return mats, names, fam, ref.cluster(mats)


def test_cluster_end_to_end(cbp):
    """M = 2T + 1 planted motifs.  PLANTED_SEED is chosen so that, on the restatement alone, no merge's mean
    lies within 1e-9 of its threshold (asserted first): a last-bit difference cannot flip a decision."""
    mats, names, fam, (comp, tree, cut) = planted_reference()
    assert len(mats) == 2 * T + 1
    assert ref.threshold_margin(cut, 0.6, 0.4) > 1e-9
    groups = {}
    for label, f in zip(cut[0], fam):
        groups.setdefault(int(label), []).append(f)
    families = sorted(g for g in groups.values() if len(g) > 1)
    assert families == [[0] * 8, [1] * 8, [2] * 8]                       # the three families, whole and alone
    assert sum(len(g) == 1 for g in groups.values()) == 9 and len(groups) == 12
    assert comp[4].sum() > 50 and len(set(comp[3].tolist())) > 5        # both strands and many offsets are in play

    timings = {}
    res = cbp.cluster(mats, timings=timings)
    assert timings["compare_ms"] > 0
    for g, w, name in zip(res.comparison, comp, NAMES):
        assert_bits(g, w, name)
    assert np.array_equal(res.tree.children, tree[0]) and res.tree.children.dtype == np.int32
    assert_bits(res.tree.distances, tree[1], "heights")
    assert np.array_equal(res.tree.sizes, tree[2])
    assert_bits(res.cut.labels, cut[0], "labels")
    assert_bits(res.cut.mean_cor, cut[1], "mean_cor")
    assert_bits(res.cut.mean_ncor, cut[2], "mean_ncor")
    assert cbp.clusters_tab(names, res.labels) == ref.clusters_tab(names, cut[0])
    # the parts compose to the whole
    again = cbp.compare(mats)
    for g, w, name in zip(again, comp, NAMES):
        assert_bits(g, w, name)
    assert np.array_equal(cbp.threshold_cut(cbp.linkage(again.dist), again.cor, again.ncor).labels, cut[0])
    one = cbp.cluster(mats[:1])
    assert one.labels.tolist() == [1] and one.tree.children.shape == (0, 2) and one.comparison.cor.size == 0


def test_refusals_come_before_the_device(cbp, monkeypatch):
    from expecto_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("the device library was asked for")
    monkeypatch.setattr(_lib, "load", no_device)
    ok = ref.random_counts(5, 1)
    neg, zero = ok.copy(), ok.copy()
    neg[2, 1] = -1.0
    zero[4] = 0.0
    for mats, msg in (([ok, np.concatenate([ref.random_counts(64, 1), ok[:1]])], "width 65"), ([ok] * 4097, "4097 motifs"),
                      ([ok, neg], "negative count"), ([zero, ok], "all zero")):
        for fn in (cbp.compare, cbp.cluster):
            with pytest.raises(ValueError, match=msg):
                fn(mats)
    with pytest.raises(ValueError, match="min_w"):
        cbp.compare([ok, ok], min_w=0)


# ---- command line --------------------------------------------------------------------------------

def check_outputs(cbp, out, motifs, min_w=5, pseudo=1.0, cor=0.6, ncor=0.4):
    """The four files of a run against the restatement of ``motifs``."""
    mats = [m.counts for m in motifs]
    comp, tree, cut = ref.cluster(mats, cor, ncor, min_w, pseudo)
    assert sorted(os.listdir(out)) == ["cluster_motifs.jaspar", "clusters_motif_names.tab", "pairwise_compa.tsv", "tree.npz"]
    assert open(out / "clusters_motif_names.tab").read() == ref.clusters_tab([m.name for m in motifs], cut[0])
    rows = [ln.split("\t") for ln in open(out / "pairwise_compa.tsv").read().splitlines()]
    assert rows[0] == ["id1", "id2", "cor", "Ncor", "strand", "offset", "w"]
    M, p = len(motifs), 0
    for i in range(M):
        for j in range(i + 1, M):
            assert rows[1 + p] == [motifs[i].id, motifs[j].id, repr(float(comp[0][p])), repr(float(comp[1][p])),
                                   "DR"[comp[4][p]], str(comp[3][p]), str(comp[5][p])]
            p += 1
    assert len(rows) == 1 + p
    z = np.load(out / "tree.npz")
    assert np.array_equal(z["children"], tree[0]) and np.array_equal(z["sizes"], tree[2])
    for key, want in (("distances", tree[1]), ("mean_cor", cut[1]), ("mean_ncor", cut[2])):
        assert_bits(z[key], want, key)
    back = cbp.read_jaspar(str(out / "cluster_motifs.jaspar"))
    assert [(m.id, m.name) for m in back] == [(m.id, m.name) for m in motifs]
    return cut[0]


def test_cli_motif_file(cbp, tmp_path):
    path = os.path.join(GOLD, "hocomoco.jaspar")
    motifs, res = cbp.main(["--motif_file", path, "--min_w", "4", "--pseudo", "0.5", "--cor", "0.55", "-o", str(tmp_path / "o")])
    assert [m.id for m in motifs] == [m.id for m in cbp.read_jaspar(path)] and len(motifs) == 5
    labels = check_outputs(cbp, tmp_path / "o", motifs, min_w=4, pseudo=0.5, cor=0.55)
    assert_bits(res.labels, labels, "labels")


def test_cli_selection_and_clustering(cbp, tmp_path, monkeypatch, capsys):
    """Stage 1 and 2 on the fixture; the tab is what predict_by_cluster reads."""
    from expecto_amd import predict_by_cluster
    monkeypatch.chdir(GOLD)                      # ./resources/*.csv
    motifs, res = cbp.main(["--belugaFeatures", "features.tsv", "--jaspar_motif_db", "jaspar",
                            "--hocomoco_jaspar_motif_file", "hocomoco.jaspar", "-o", str(tmp_path / "o")])
    assert capsys.readouterr().out.splitlines()[-1] == "Found 4 motifs out of 5 motifs in hgnc df"
    assert len(motifs) == 6
    labels = check_outputs(cbp, tmp_path / "o", motifs)
    assert_bits(res.labels, labels, "labels")
    # the two MAX, the two CTCF (one reverse complemented) and Jun with FOS were written to pair up
    assert labels.tolist() == [1, 2, 3, 1, 3, 2]
    assays = ["MAX", "JUN", "CTCF", "FOS", "ZNF274"]
    assay_clusters, table = predict_by_cluster.rsat_clusters(str(tmp_path / "o" / "clusters_motif_names.tab"), assays)
    assert assay_clusters == [[1], [3], [2], [3], [-1]]
    assert table.loc["cluster_2", 1] == "CTCF,ctcf_MOUSE.H11MO.0.A" and table.loc["cluster_-1", 1] == "ZNF274"
