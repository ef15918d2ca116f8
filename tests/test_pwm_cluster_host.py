"""The host half of the motif similarity clustering, without a GPU: expecto_amd/csrc/average_linkage.h
(built with the host compiler alone into tests/average_linkage_driver.cpp, as test_ward_host.py builds
the Ward header) against the restatement (tests/pwm_cluster_ref.py) and, where it is installed, scipy;
the JASPAR reader and writer; and the motif selection of cluster_by_pwm.py:52-72 on the hand-made
fixture tests/golden/cluster_by_pwm/."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import pwm_cluster_ref as ref
from expecto_amd import cluster_by_pwm as cbp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "average_linkage_driver.cpp")
GOLD = os.path.join(REPO, "tests", "golden", "cluster_by_pwm")

CASES = {f"gamma-{n}": ("gamma", n) for n in (2, 3, 37, 130)}
CASES["ties-40"] = ("ties", 40)


@functools.lru_cache(maxsize=None)
def distances(name):
    kind, n = CASES[name]
    D = ref.gamma_distances(n) if kind == "gamma" else ref.tie_distances(n)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def reference(name):
    out = ref.linkage(distances(name), CASES[name][1])
    for a in out:
        a.setflags(write=False)
    return out


def _cxx():
    return [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("avg") / "average_linkage_driver")
    subprocess.run(_cxx() + ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", SRC, "-o", exe], check=True)
    return exe


def _hex(values):
    return " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in values)


def linkage_case(n, cond):
    return f"linkage {n}\n{_hex(cond)}\n"


def cut_case(n, children, cor, ncor, min_cor, min_ncor):
    return (f"cut {n} {_hex([min_cor, min_ncor])}\n{' '.join(str(int(c)) for c in np.asarray(children).ravel())}\n"
            f"{_hex(cor)}\n{_hex(ncor)}\n")


def run_driver(exe, cases):
    """Case texts -> per case the error text, a tree (children, heights, sizes) or a cut (labels, mean_cor, mean_ncor)."""
    out = subprocess.run([exe], input="".join(cases), capture_output=True, text=True, check=True).stdout
    res, cur = [], None
    for ln in out.splitlines():
        word, _, rest = ln.partition(" ")
        if word == "case":
            cur = {"merge": [], "mean": [], "labels": None, "error": None}
        elif word == "error":
            cur["error"] = rest
        elif word == "merge":
            a, b, h, s = rest.split()
            cur["merge"].append((int(a), int(b), float.fromhex(h), int(s)))
        elif word == "labels":
            cur["labels"] = np.array(rest.split(), np.int32)
        elif word == "mean":
            cur["mean"].append([float.fromhex(v) for v in rest.split()])
        elif word == "end":
            if cur["error"] is not None:
                res.append(cur["error"])
            elif cur["labels"] is not None:
                mean = np.array(cur["mean"], np.float64).reshape(-1, 2)
                res.append((cur["labels"], mean[:, 0].copy(), mean[:, 1].copy()))
            else:
                m = cur["merge"]
                res.append((np.array([r[:2] for r in m], np.int64).reshape(len(m), 2), np.array([r[2] for r in m], np.float64),
                            np.array([r[3] for r in m], np.int64)))
    assert len(res) == len(cases)
    return res


def assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, k)
        if g.dtype.kind == "f":
            assert np.array_equal(g.view(np.uint64), np.asarray(w, np.float64).view(np.uint64)), (what, k)
        else:
            assert np.array_equal(g, w), (what, k)


# ---- average linkage -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_driver_equals_restatement(driver, name):
    got, = run_driver(driver, [linkage_case(CASES[name][1], distances(name))])
    assert_same(got, reference(name), name)


def test_ties_are_tie_heavy():
    cond, (_, heights, _) = distances("ties-40"), reference("ties-40")
    assert set(np.unique(cond)) <= {0.0, 0.25, 0.5, 1.0} and (cond == 0).sum() >= 2
    assert len(heights) - len(np.unique(heights)) >= 10


@pytest.mark.parametrize("name", list(CASES))
def test_scipy_average_bitwise(driver, name):
    pytest.importorskip("scipy")
    from scipy.cluster.hierarchy import linkage
    Z = linkage(np.array(distances(name)), method='average')
    scipy_tree = (Z[:, :2].astype(np.int64), Z[:, 2], Z[:, 3].astype(np.int64))
    assert_same(reference(name), scipy_tree, name + " restatement vs scipy")
    got, = run_driver(driver, [linkage_case(CASES[name][1], distances(name))])
    assert_same(got, scipy_tree, name + " driver vs scipy")


def test_linkage_refusals(driver):
    nan = np.array([1.0, np.nan, 2.0])
    inf = np.array([np.inf, np.inf, 1.0])
    got = run_driver(driver, [linkage_case(1, []), linkage_case(0, []), linkage_case(3, nan), linkage_case(3, inf)])
    assert got == ["average linkage needs at least 2 points", "average linkage needs at least 2 points",
                   "average linkage: NaN in the distance matrix",
                   "average linkage: a cluster has no neighbour at a finite distance"]
    for n, cond, text in ((1, [], "at least 2 points"), (3, nan, "NaN in the distance matrix")):
        with pytest.raises(ValueError, match=text):
            ref.linkage(cond, n)


# ---- threshold cut -------------------------------------------------------------------------------

def pair_scores(n, value):
    """Condensed scores from value(i, j)."""
    return np.array([value(i, j) for i in range(n) for j in range(i + 1, n)], np.float64)


# leaves 0..4; merges: 5 = (1, 3), 6 = (0, 4), 7 = (2, 5), 8 = (6, 7)
HAND_TREE = np.array([[1, 3], [0, 4], [2, 5], [6, 7]], np.int64)


def hand_cut(driver, cor, ncor, min_cor=0.6, min_ncor=0.4):
    want = ref.threshold_cut(HAND_TREE, 5, cor, ncor, min_cor, min_ncor)
    got, = run_driver(driver, [cut_case(5, HAND_TREE, cor, ncor, min_cor, min_ncor)])
    assert_same(got, want, "hand tree")
    return got


def test_cut_all_accepted_is_one_cluster(driver):
    labels, mean_cor, mean_ncor = hand_cut(driver, pair_scores(5, lambda i, j: 0.9), pair_scores(5, lambda i, j: 0.7))
    assert labels.tolist() == [1] * 5
    assert mean_cor.tolist() == [0.9, 0.9, (0.9 + 0.9) / 2.0, ((((0.9 + 0.9) + 0.9) + 0.9) + 0.9 + 0.9) / 6.0]


def test_cut_none_accepted_is_singletons(driver):
    for cor, ncor in ((0.9, 0.1), (0.1, 0.9)):         # either threshold alone rejects
        labels, _, _ = hand_cut(driver, pair_scores(5, lambda i, j: cor), pair_scores(5, lambda i, j: ncor))
        assert labels.tolist() == [1, 2, 3, 4, 5]


def test_cut_rejected_child_keeps_its_parent_rejected(driver):
    """Merge 5 = (1, 3) fails; merge 7 = (2, 5) has passing means (pairs (1, 2) and (2, 3)) and stays rejected,
    and so does the root.  Merge 6 = (0, 4) holds.  Labels by smallest member: {0, 4} 1, {1} 2, {2} 3, {3} 4."""
    low = {(1, 3)}
    cor = pair_scores(5, lambda i, j: 0.2 if (i, j) in low else 0.9)
    labels, mean_cor, mean_ncor = hand_cut(driver, cor, cor)
    assert mean_cor[0] == 0.2 and mean_cor[2] == 0.9 and mean_cor[3] >= 0.6
    assert labels.tolist() == [1, 2, 3, 4, 1]


def test_cut_label_numbering_and_thresholds_are_inclusive(driver):
    """{1, 3} and {0, 4} hold with means exactly at the thresholds; the rest fails: 0 -> 1, 1 -> 2, 2 -> 3."""
    keep = {(1, 3), (0, 4)}
    cor = pair_scores(5, lambda i, j: 0.6 if (i, j) in keep else 0.0)
    ncor = pair_scores(5, lambda i, j: 0.4 if (i, j) in keep else 0.0)
    labels, _, _ = hand_cut(driver, cor, ncor)
    assert labels.tolist() == [1, 2, 3, 2, 1]
    labels, _, _ = hand_cut(driver, cor, ncor, min_cor=np.nextafter(0.6, 1.0))
    assert labels.tolist() == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("name", ["gamma-37", "ties-40"])
def test_cut_of_linkage_trees_equals_restatement(driver, name):
    n = CASES[name][1]
    children = reference(name)[0]
    rng = np.random.default_rng(n)
    cor, ncor = rng.uniform(-0.2, 1.0, n * (n - 1) // 2), rng.uniform(-0.2, 1.0, n * (n - 1) // 2)
    cases = [(0.3, 0.2), (0.5, 0.4), (-1.0, -1.0), (2.0, 2.0)]
    got = run_driver(driver, [cut_case(n, children, cor, ncor, a, b) for a, b in cases])
    for g, (a, b) in zip(got, cases):
        assert_same(g, ref.threshold_cut(children, n, cor, ncor, a, b), (name, a, b))
    assert got[2][0].tolist() == [1] * n and got[3][0].tolist() == list(range(1, n + 1))
    assert 1 < got[0][0].max() < n


def test_cut_refusals(driver):
    z = np.zeros(3)
    got = run_driver(driver, [cut_case(1, [], [], [], 0.6, 0.4), cut_case(3, [[0, 1], [0, 2]], z, z, 0.6, 0.4),
                              cut_case(3, [[0, 3], [1, 2]], z, z, 0.6, 0.4)])
    assert got[0] == "average linkage needs at least 2 points"
    assert got[1].startswith("threshold cut: children is not a tree") and got[2] == got[1]


def test_driver_under_sanitizers(tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined and run directly: same output, no report."""
    exe = str(tmp_path / "average_linkage_driver_san")
    build = subprocess.run(_cxx() + ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                     "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the host compiler has no address/undefined sanitizer runtime: " + build.stderr[-200:])
    names = list(CASES)
    z = np.zeros(3)
    cor = pair_scores(5, lambda i, j: 0.2 if (i, j) == (1, 3) else 0.9)
    got = run_driver(exe, [linkage_case(CASES[k][1], distances(k)) for k in names] +
                     [cut_case(5, HAND_TREE, cor, cor, 0.6, 0.4), cut_case(3, [[0, 3], [1, 2]], z, z, 0.6, 0.4),
                      linkage_case(1, [])])
    for k, g in zip(names, got):
        assert_same(g, reference(k), k + " under sanitizers")
    assert_same(got[len(names)], ref.threshold_cut(HAND_TREE, 5, cor, cor, 0.6, 0.4), "cut under sanitizers")
    assert got[-2].startswith("threshold cut") and got[-1] == "average linkage needs at least 2 points"


# ---- JASPAR text ---------------------------------------------------------------------------------

def test_jaspar_round_trip():
    motifs = [cbp.Motif("MA0001.1", "MA0001.1", np.array([[3.0, 0.0, 1.0, 0.0]])),                      # no name, width 1
              cbp.Motif("MA0059.1", "MAX::MYC", ref.random_counts(7, 1)),
              cbp.Motif("FOS_HUMAN.H11MO.0.A", "FOS_HUMAN.H11MO.0.A", ref.random_counts(12, 2) + 0.25)]
    text = cbp.format_jaspar(motifs)
    assert text.splitlines()[0] == ">MA0001.1 MA0001.1" and text.splitlines()[1] == "A [  3.00]"
    assert text.splitlines()[6] == "A [" + " ".join("%6.2f" % v for v in motifs[1].counts[:, 0]) + "]"
    back = cbp.parse_jaspar(text)
    assert [(m.id, m.name) for m in back] == [(m.id, m.name) for m in motifs]
    for b, m in zip(back, motifs):
        assert b.counts.dtype == np.float64 and np.array_equal(b.counts, m.counts)
    # the file as the CLI writes it (print adds an empty line) reads back the same
    assert [m.id for m in cbp.parse_jaspar(text + "\n")] == [m.id for m in motifs]


def test_jaspar_reader_forms():
    got = cbp.parse_jaspar(">X1\nA  [ 1 2 ]\nC [3 4]\nG\t[ 5\t6 ]\nT 7 8\n\n>X2   named  extra words\nT [0]\nG [0]\nC [2]\nA [1]\n")
    assert [(m.id, m.name) for m in got] == [("X1", "X1"), ("X2", "named")]
    assert got[0].counts.tolist() == [[1, 3, 5, 7], [2, 4, 6, 8]] and got[1].counts.tolist() == [[1, 2, 0, 0]]
    for text, msg in ((">X\nA [1]\nC [1]\nG [1]\n", "not one each"), (">X\nA [1 2]\nC [1]\nG [1]\nT [1]\n", "rows of"),
                      ("A [1]\n", "cannot read"), (">X\nA [1]\nA [2]\n", "two A rows"), (">X\nA [x]\n", "no number")):
        with pytest.raises(ValueError, match=msg):
            cbp.parse_jaspar(text)


def test_jaspar_directory_takes_one_motif_per_file(tmp_path):
    one = cbp.format_jaspar([cbp.Motif("B", "b", ref.random_counts(3, 1))])
    (tmp_path / "b.jaspar").write_text(one)
    (tmp_path / "a.jaspar").write_text(cbp.format_jaspar([cbp.Motif("A", "a", ref.random_counts(2, 1))]))
    (tmp_path / "ignored.txt").write_text("not a motif")
    assert [m.id for m in cbp.read_jaspar_dir(str(tmp_path))] == ["A", "B"]
    (tmp_path / "c.jaspar").write_text(one + one)
    with pytest.raises(ValueError, match="more than one motif found in .*c.jaspar"):
        cbp.read_jaspar_dir(str(tmp_path))


def test_meme_motif_file(tmp_path):
    (tmp_path / "m.meme").write_text("MEME version 4\n\nALPHABET= ACGT\n\nMOTIF ID0 ALT0\nletter-probability matrix: alength= 4 "
                                     "w= 2 nsites= 8\n0.5 0.25 0.25 0\n0 0 0 1\n\nMOTIF ID1\nletter-probability matrix: "
                                     "alength= 4 w= 1\n0.25 0.25 0.25 0.25\n")
    got = cbp.read_motif_file(str(tmp_path / "m.meme"))
    assert [(m.id, m.name) for m in got] == [("ID0", "ALT0"), ("ID1", "ID1")]
    assert got[0].counts.tolist() == [[4, 2, 2, 0], [0, 0, 0, 8]] and got[1].counts.tolist() == [[5, 5, 5, 5]]


# ---- selection -----------------------------------------------------------------------------------

def test_selection_on_the_fixture(monkeypatch, tmp_path, capsys):
    """By hand from cluster_by_pwm.py:32-72.  Marks: DNase and H3K4me3 go by assay type, Pol2 by its name,
    p300 maps to EP300, which Lambert's list lacks; Max (twice), c-Jun, CTCF, c-Fos and ZNF274 stay, as MAX,
    JUN, CTCF, FOS, ZNF274: 5 names.  JASPAR, files in sorted order: MA0003.1 has no name (its id is none of
    them), MA0058.1 MAX stays, MA0059.1 MAX::MYC is a heterodimer, MA0106.1 TP53 is no mark, MA0139.1 CTCF
    and MA0488.1 Jun stay.  HOCOMOCO: MAX_HUMAN and FOS_HUMAN stay, P53 is no mark, ZN274 is not ZNF274,
    ctcf_MOUSE stays.  Found: MAX, CTCF, JUN, FOS."""
    monkeypatch.chdir(GOLD)                      # ./resources/*.csv
    args = cbp.build_parser().parse_args(["--belugaFeatures", "features.tsv", "--jaspar_motif_db", "jaspar",
                                          "--hocomoco_jaspar_motif_file", "hocomoco.jaspar", "--cisbp2_meme_file",
                                          "missing.meme", "--no_cluster", "-o", str(tmp_path / "out")])
    motifs, res = cbp.run(args)
    assert res is None
    assert [m.id for m in motifs] == ["MA0058.1", "MA0139.1", "MA0488.1", "MAX_HUMAN.H11MO.0.A", "FOS_HUMAN.H11MO.0.A",
                                      "ctcf_MOUSE.H11MO.0.A"]
    assert [m.name for m in motifs[:3]] == ["MAX", "CTCF", "Jun"] and all(m.name == m.id for m in motifs[3:])
    out = capsys.readouterr().out.splitlines()
    assert out == ["not including DNase features", "not including histone features", "intersecting with Lambert data",
                   "taking out Pol2*", "Found 4 motifs out of 5 motifs in hgnc df"]
    assert sorted(os.listdir(tmp_path / "out")) == ["cluster_motifs.jaspar"]
    back = cbp.read_jaspar(str(tmp_path / "out" / "cluster_motifs.jaspar"))
    assert [(m.id, m.name) for m in back] == [(m.id, m.name) for m in motifs]
    for b, m in zip(back, motifs):
        assert np.array_equal(b.counts, m.counts)
    assert motifs[2].counts[:, 3].tolist() == [17, 1, 1, 1, 19, 0, 1] and motifs[5].counts.shape == (9, 4)
    assert cbp.kept_assays("features.tsv").tolist() == ["MAX", "JUN", "CTCF", "FOS", "MAX", "ZNF274"]


# ---- checks before the device --------------------------------------------------------------------

def test_frequencies_and_refusals():
    mats = [ref.random_counts(w, w) for w in (1, 5, 64)]
    mats[1][2] = [0.0, 0.0, 3.0, 0.0]
    freq, col_ptr = cbp.frequencies(mats, 0.5)
    assert col_ptr.tolist() == [0, 1, 6, 70] and freq.shape == (70, 4)
    assert np.abs(freq.sum(axis=1) - 1.0).max() < 1e-15
    assert np.array_equal((freq - 0.25).ravel().view(np.uint64),
                          np.array(sum((ref.frequencies(m, 0.5) for m in mats), [])).view(np.uint64))
    ok = ref.random_counts(4, 1)
    bad = ok.copy()
    bad[1, 2] = -1.0
    zero = ok.copy()
    zero[3] = 0.0
    nan = ok.copy()
    nan[0, 0] = np.nan
    for mats, msg in (([ok, ref.random_counts(64, 1)[np.r_[0:64, 0]]], "motif 1: width 65"), ([ok] * 4097, "4097 motifs"),
                      ([ok, bad], "motif 1: a negative count"), ([zero], "motif 0: column 3 is all zero"),
                      ([nan], "NaN or infinite"), ([ok[:, :3]], r"shape \(4, 3\)"), ([ok[:0]], "width 0")):
        with pytest.raises(ValueError, match=msg):
            cbp.frequencies(mats)
    with pytest.raises(ValueError, match="pseudo"):
        cbp.frequencies([ok], -1.0)


def test_files():
    assert cbp.clusters_tab(["a", "B_x", "c", "d"], [2, 1, 2, 3]) == "cluster_1\tB_x\ncluster_2\ta,c\ncluster_3\td\n"
    comp = cbp.Comparison(np.array([0.5, -0.25, 1.0]), np.array([0.25, -0.125, 1.0]), np.array([0.75, 1.125, 0.0]),
                          np.array([-2, 0, 3], np.int32), np.array([0, 1, 0], np.int32), np.array([5, 6, 7], np.int32))
    assert cbp.pairwise_table(["x", "y", "z"], comp).splitlines() == [
        "id1\tid2\tcor\tNcor\tstrand\toffset\tw", "x\ty\t0.5\t0.25\tD\t-2\t5", "x\tz\t-0.25\t-0.125\tR\t0\t6",
        "y\tz\t1.0\t1.0\tD\t3\t7"]
