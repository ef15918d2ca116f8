"""Batched k-means on the device: the kernels of csrc/kmeans.hip through their C entry points,
``cluster_and_viz.kmeans`` / ``kmeans_sweep`` and the CLI.

Both kernels run one workgroup of 1024 lanes per problem, four points per lane at most; the chains
load 8 terms ahead, the E-step takes 8 centres per pass and ``2048 // d`` centres per LDS chunk.  The
shapes below sit on both sides of those steps.  Outputs lie in pattern-filled buffers
(tests/guarded.py) and X inside NaN margins with NaN row padding (``ld > d``), so a store outside an
output or a load outside the matrix fails the test.  Every comparison with the restatement
(tests/kmeans_ref.py) is bitwise."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import kmeans_ref
from conftest import GOLDEN
from guarded import Guarded, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

FEATURES_TSV = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
COLS = 8


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


class Rows64:
    """float64 [n, d] on the device with row stride ld; NaN padding, NaN margins before and after."""

    def __init__(self, X, ld, margin=64):
        X = np.asarray(X, np.float64)
        n, d = X.shape
        host = np.full(margin + n * ld + margin, np.nan)
        host[margin:margin + n * ld].reshape(n, ld)[:, :d] = X
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + 8 * margin
        self.n, self.d, self.ld = n, d, ld


def table(rows):
    t = np.zeros((len(rows), COLS), np.int64)
    for p, r in enumerate(rows):
        t[p, :len(r)] = r
    return t


def workspace(lib, n, d, k_max, t_max, P):
    nbytes = int(lib.expecto_kmeans_workspace(n, d, k_max, t_max, P))
    assert nbytes > 0
    return Guarded((nbytes // 8,), np.float64), nbytes


def seed_device(lib, X, problems, ld=None):
    """problems: [(k, first, u [k-1, T])] -> [(idx, centres)]."""
    n, d = X.shape
    src = Rows64(X, ld or d + 3)
    ks = [p[0] for p in problems]
    Ts = [np.asarray(p[2]).reshape(p[0] - 1, -1).shape[1] if p[0] > 1 else 1 for p in problems]
    c_off = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    u_off = np.concatenate([[0], np.cumsum([(k - 1) * T for k, T in zip(ks, Ts)])]).astype(np.int64)
    tab = table([(k, p[1], T, u_off[i], c_off[i], c_off[i]) for i, (p, k, T) in enumerate(zip(problems, ks, Ts))])
    u = np.concatenate([np.asarray(p[2], np.float64).ravel() for p in problems] + [np.zeros(1)])
    d_tab, d_u = dev(tab), dev(u)
    idx, cen = Guarded((int(c_off[-1]),), np.int32), Guarded((int(c_off[-1]), d), np.float64)
    ws, nbytes = workspace(lib, n, d, max(ks), max(Ts), len(problems))
    st = lib.expecto_kmeans_plusplus(src.ptr, n, d, src.ld, len(problems), tab.ctypes.data, d_tab.data_ptr(),
                                     d_u.data_ptr(), idx.ptr, cen.ptr, ws.ptr, nbytes, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    ws.result()
    idx, cen = idx.result(), cen.result()
    return [(idx[c_off[i]:c_off[i + 1]], cen[c_off[i]:c_off[i + 1]]) for i in range(len(problems))]


def lloyd_device(lib, X, problems, ld=None):
    """problems: [(C0 [k, d], tol, max_iter)] -> [(labels, centres, inertia, n_iter)]."""
    n, d = X.shape
    src = Rows64(X, ld or d + 3)
    ks = [np.asarray(p[0]).shape[0] for p in problems]
    c_off = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    tab = table([(k, p[2], c_off[i], c_off[i], i * n) for i, (p, k) in enumerate(zip(problems, ks))])
    init = np.concatenate([np.asarray(p[0], np.float64).reshape(-1, d) for p in problems])
    d_tab, d_init, d_tol = dev(tab), dev(init), dev(np.array([p[1] for p in problems], np.float64))
    P = len(problems)
    lab, cen = Guarded((P, n), np.int32), Guarded((int(c_off[-1]), d), np.float64)
    inertia, n_iter = Guarded((P,), np.float64), Guarded((P,), np.int32)
    ws, nbytes = workspace(lib, n, d, max(ks), 1, P)
    st = lib.expecto_kmeans_lloyd(src.ptr, n, d, src.ld, P, tab.ctypes.data, d_tab.data_ptr(), d_tol.data_ptr(),
                                  d_init.data_ptr(), lab.ptr, cen.ptr, inertia.ptr, n_iter.ptr, ws.ptr, nbytes, ST())
    assert st == 0, lib.expecto_last_error().decode()
    torch.cuda.synchronize()
    ws.result()
    lab, cen, inertia, n_iter = lab.result(), cen.result(), inertia.result(), n_iter.result()
    return [(lab[i], cen[c_off[i]:c_off[i + 1]], inertia[i], n_iter[i]) for i in range(P)]


def assert_seed(got, want, what):
    assert_bits(got[0], want[0], what + " idx")
    assert_bits(got[1], want[1], what + " centres")


def assert_lloyd(got, want, what):
    assert_bits(got[0], want[0], what + " labels")
    assert_bits(got[1], want[1], what + " centres")
    assert_bits(np.float64(got[2]), np.float64(want[2]), what + " inertia")
    assert int(got[3]) == int(want[3]), (what, "n_iter", int(got[3]), int(want[3]))


@functools.lru_cache(maxsize=None)
def points(n, d, seed=3):
    X = kmeans_ref.blobs(n, d, 5, seed)
    X.setflags(write=False)
    return X


def uniforms(k, T, seed):
    return np.random.RandomState(seed).uniform(size=(k - 1, T))


def ks_of(n):
    return sorted({k for k in (1, 2, 7, 64, 65, n) if k <= min(n, 512)})


# (n, d): every n with a small d; every d with n on both sides of a wave; one case past a workgroup's lanes
SHAPES = [(1, 3), (2, 3), (63, 3), (64, 1), (65, 20), (257, 3), (65, 33), (64, 100), (1025, 3)]


@pytest.mark.parametrize("n,d", SHAPES)
def test_seeding_shapes(lib, n, d):
    X = points(n, d)
    problems = [(k, (3 * k) % n, uniforms(k, min(8, kmeans_ref.trials(k)), k)) for k in ks_of(n)]
    want = [kmeans_ref.plusplus(X, *p) for p in problems]
    got = seed_device(lib, X, problems)
    for p, g, w in zip(problems, got, want):
        assert_seed(g, w, f"n={n} d={d} k={p[0]}")
        assert_bits(g[1], X[g[0]], "centres are rows of X")


@pytest.mark.parametrize("n,d", SHAPES)
def test_lloyd_shapes(lib, n, d):
    X = points(n, d)
    problems = []
    for k in ks_of(n):
        _, C0 = kmeans_ref.plusplus(X, k, (3 * k) % n, uniforms(k, kmeans_ref.trials(k), k))
        problems.append((C0, kmeans_ref.tolerance(X), 300))
    got = lloyd_device(lib, X, problems)
    for p, g in zip(problems, got):
        assert_lloyd(g, kmeans_ref.lloyd(X, *p), f"n={n} d={d} k={p[0].shape[0]}")
    if n == 1:
        assert int(got[0][3]) <= 2


def test_large_k_and_t(lib):
    """k = 512 of n = 600 with T = 8, d = 5: the limits of k and T, several E-step chunks at d = 100."""
    X = points(600, 5)
    p = (512, 17, uniforms(512, 8, 1))
    g, = seed_device(lib, X, [p])
    assert_seed(g, kmeans_ref.plusplus(X, *p), "k=512")
    got, = lloyd_device(lib, X, [(g[1], 0.0, 5)])
    assert_lloyd(got, kmeans_ref.lloyd(X, g[1], 0.0, 5), "k=512")
    X = points(130, 100)
    C0 = X[::2][:65].copy()      # 65 centres of d = 100: chunks of 20
    got, = lloyd_device(lib, X, [(C0, 0.0, 4)])
    assert_lloyd(got, kmeans_ref.lloyd(X, C0, 0.0, 4), "d=100 chunks")


def grid_points():
    """Points on a 3 x 3 integer grid, each several times: distances tie exactly."""
    rng = np.random.RandomState(4)
    return rng.randint(0, 3, size=(90, 2)).astype(np.float64)


def test_ties(lib):
    X = grid_points()
    # centres midway between grid points: every point on the middle line ties between two centres
    C0 = np.array([[0.5, 1.0], [1.5, 1.0], [0.5, 1.0], [1.0, 0.5], [1.0, 1.5]])
    for max_iter in (1, 2, 50):
        got, = lloyd_device(lib, X, [(C0, 0.0, max_iter)])
        want = kmeans_ref.lloyd(X, C0, 0.0, max_iter)
        assert_lloyd(got, want, f"grid max_iter={max_iter}")
    lab, dist = kmeans_ref.e_step(X, C0)
    assert (np.sort(kmeans_ref.d2(X, C0), axis=1)[:, 0] == np.sort(kmeans_ref.d2(X, C0), axis=1)[:, 1]).any()
    assert not (lab == 2).any()          # the duplicate centre never wins: an empty cluster, relocation with tied dist
    # seeding on duplicates: zero distances inside cum, duplicate candidates in a step
    u = np.array([[0.3, 0.3, 0.3001], [0.0, 0.99, 0.5], [0.7, 0.7, 0.7], [0.1, 0.2, 0.1]])
    g, = seed_device(lib, X, [(5, 4, u)])
    assert_seed(g, kmeans_ref.plusplus(X, 5, 4, u), "grid seeding")


def test_empty_clusters(lib):
    X = points(257, 3)
    base = X[[5, 50, 100]].copy()
    far = np.full((1, 3), 1e6)
    cases = {
        "duplicate centre": np.vstack([base, base[1:2]]),
        "far centre": np.vstack([base[:1], far, base[1:]]),
        "several": np.vstack([far, base[:1], base[:1], far + 1, base[1:], base[:1], far + 2]),
        "all but one": np.vstack([base[:1]] * 64),
    }
    problems = [(C0, kmeans_ref.tolerance(X), m) for C0 in cases.values() for m in (1, 300)]
    got = lloyd_device(lib, X, problems)
    for (name, m), p, g in zip(((c, m) for c in cases for m in (1, 300)), problems, got):
        lab0, _ = kmeans_ref.e_step(X, p[0])
        assert (np.bincount(lab0, minlength=p[0].shape[0]) == 0).any(), name
        assert_lloyd(g, kmeans_ref.lloyd(X, *p), f"{name} max_iter={m}")


def test_stops(lib):
    X = points(257, 3)
    _, C0 = kmeans_ref.plusplus(X, 7, 1, uniforms(7, 3, 9))
    problems = [(C0, 0.0, 1), (C0, 0.0, 2), (C0, 0.0, 300), (C0, 1e300, 300), (C0, kmeans_ref.tolerance(X), 300)]
    got = lloyd_device(lib, X, problems)
    for p, g in zip(problems, got):
        assert_lloyd(g, kmeans_ref.lloyd(X, *p), f"tol={p[1]} max_iter={p[2]}")
    assert [int(g[3]) for g in got[:2]] == [1, 2] and int(got[3][3]) == 1 and int(got[2][3]) > 2


def test_batches(lib):
    """Problems of different k in one call equal each alone; two identical calls give identical bits."""
    X = points(257, 20)
    seeds = [(k, (5 * k) % 257, uniforms(k, kmeans_ref.trials(k), k)) for k in (2, 65, 7, 1, 64)]
    batch = seed_device(lib, X, seeds)
    again = seed_device(lib, X, seeds)
    for p, b, a in zip(seeds, batch, again):
        assert_seed(b, a, "second call")
        assert_seed(b, seed_device(lib, X, [p])[0], f"alone k={p[0]}")
    problems = [(b[1], kmeans_ref.tolerance(X), 300) for b in batch]
    got = lloyd_device(lib, X, problems)
    again = lloyd_device(lib, X, problems)
    for p, g, a in zip(problems, got, again):
        assert_lloyd(g, a, "second call")
        assert_lloyd(g, lloyd_device(lib, X, [p])[0], f"alone k={p[0].shape[0]}")
        assert_lloyd(g, kmeans_ref.lloyd(X, *p), f"k={p[0].shape[0]}")


def test_many_problems(lib):
    """300 problems of n = 65: more workgroups than compute units."""
    X = points(65, 3)
    seeds = [(2 + p % 9, p % 65, uniforms(2 + p % 9, kmeans_ref.trials(2 + p % 9), p)) for p in range(300)]
    got = seed_device(lib, X, seeds)
    want = [kmeans_ref.plusplus(X, *p) for p in seeds]
    for i, (g, w) in enumerate(zip(got, want)):
        assert_seed(g, w, f"problem {i}")
    problems = [(w[1], 0.0, 300) for w in want]
    for i, (g, p) in enumerate(zip(lloyd_device(lib, X, problems), problems)):
        assert_lloyd(g, kmeans_ref.lloyd(X, *p), f"problem {i}")


def test_seeding_edges(lib):
    """u = 0 takes the first point; u just below 1 with a product that rounds past cum[n-1] is clipped
    to n - 1; duplicate candidates within a step."""
    X = points(65, 3)
    top = np.nextafter(1.0, 0.0)
    u = np.array([[0.0, top, 0.5], [top, top, top], [0.0, 0.0, 0.0], [0.25, 0.25, top]])
    g, = seed_device(lib, X, [(5, 64, u)])
    assert_seed(g, kmeans_ref.plusplus(X, 5, 64, u), "edges")
    # a pot the chain rounds below top * pot never exists (top * pot <= pot), so clipping is forced with
    # values of u at 1.0 and above, which sklearn's clip handles the same way
    u = np.array([[1.0, 2.0, 0.5]])
    g, = seed_device(lib, X, [(2, 0, u)])
    want = kmeans_ref.plusplus(X, 2, 0, u)
    assert_seed(g, want, "clipped")


def test_nothing_to_do_and_refusals(lib):
    X = points(65, 3)
    src = Rows64(X, 4)
    n, d = 65, 3
    out_i, out_c = Guarded((16,), np.int32), Guarded((16, d), np.float64)
    lab, inertia, n_iter = Guarded((2, n), np.int32), Guarded((2,), np.float64), Guarded((2,), np.int32)
    ws, nbytes = workspace(lib, n, d, 8, 8, 2)
    assert lib.expecto_kmeans_plusplus(None, n, d, d, 0, None, None, None, None, None, None, 0, ST()) == 0
    assert lib.expecto_kmeans_lloyd(None, n, d, d, 0, None, None, None, None, None, None, None, None, None, 0, ST()) == 0
    u, tol, init = dev(np.full(64, 0.5)), dev(np.zeros(2)), dev(np.array(X[:16]))
    good = table([(3, 1, 2, 0, 0, 0), (2, 5, 2, 4, 3, 3)])
    d_good = dev(good)

    def seed(tab=good, **k):
        a = dict(X=src.ptr, n=n, d=d, ld=4, P=2, host=tab.ctypes.data, dev=d_good.data_ptr(), u=u.data_ptr(),
                 idx=out_i.ptr, cen=out_c.ptr, ws=ws.ptr, nbytes=nbytes)
        a.update(k)
        return lib.expecto_kmeans_plusplus(*a.values(), ST())

    def bad(row, col, v):
        t = good.copy()
        t[row, col] = v
        return t

    for kw, text in ((dict(tab=bad(0, 0, 0)), "k must lie"), (dict(tab=bad(0, 0, 513)), "k must lie"),
                     (dict(tab=bad(0, 0, 66)), "k > n"), (dict(tab=bad(0, 2, 9)), "T must lie"),
                     (dict(tab=bad(0, 2, 0)), "T must lie"), (dict(tab=bad(1, 1, 65)), "first outside"),
                     (dict(tab=bad(1, 1, -1)), "first outside"), (dict(tab=bad(0, 3, 1)), "inconsistent offsets"),
                     (dict(tab=bad(1, 4, 2)), "inconsistent offsets"), (dict(tab=bad(1, 5, -1)), "inconsistent offsets"),
                     (dict(ld=2), "ld < d"), (dict(n=4097), "n must lie"), (dict(n=0), "n must lie"),
                     (dict(d=129), "d must lie"), (dict(P=-1), "problem count"), (dict(X=None), "null argument"),
                     (dict(host=None), "null argument"), (dict(idx=None), "null argument"),
                     (dict(ws=None), "null argument"), (dict(nbytes=64), "workspace too small")):
        tab = kw.pop("tab", good)
        assert seed(tab, **kw) == -1, (kw, text)
        assert text in lib.expecto_last_error().decode(), (kw, text)

    lgood = table([(3, 5, 0, 0, 0), (2, 5, 3, 3, n)])
    d_lgood = dev(lgood)

    def lloyd(tab=lgood, **k):
        a = dict(X=src.ptr, n=n, d=d, ld=4, P=2, host=tab.ctypes.data, dev=d_lgood.data_ptr(), tol=tol.data_ptr(),
                 init=init.data_ptr(), lab=lab.ptr, cen=out_c.ptr, inertia=inertia.ptr, n_iter=n_iter.ptr, ws=ws.ptr,
                 nbytes=nbytes)
        a.update(k)
        return lib.expecto_kmeans_lloyd(*a.values(), ST())

    def lbad(row, col, v):
        t = lgood.copy()
        t[row, col] = v
        return t

    for kw, text in ((dict(tab=lbad(0, 0, 0)), "k must lie"), (dict(tab=lbad(1, 0, 66)), "k > n"),
                     (dict(tab=lbad(0, 1, 0)), "max_iter"), (dict(tab=lbad(0, 2, 1)), "inconsistent offsets"),
                     (dict(tab=lbad(1, 3, 2)), "inconsistent offsets"), (dict(tab=lbad(1, 4, n - 1)), "inconsistent offsets"),
                     (dict(ld=2), "ld < d"), (dict(tol=None), "null argument"), (dict(init=None), "null argument"),
                     (dict(lab=None), "null argument"), (dict(inertia=None), "null argument"),
                     (dict(nbytes=8), "workspace too small")):
        tab = kw.pop("tab", lgood)
        assert lloyd(tab, **kw) == -1, (kw, text)
        assert text in lib.expecto_last_error().decode(), (kw, text)
    assert lib.expecto_kmeans_workspace(4097, 3, 2, 2, 1) == 0 and lib.expecto_kmeans_workspace(65, 3, 513, 2, 1) == 0
    torch.cuda.synchronize()
    for g in (out_i, out_c, lab, inertia, n_iter, ws):
        assert g.untouched()
    # the good tables do run
    assert seed() == 0 and lloyd() == 0
    torch.cuda.synchronize()
    assert not out_i.untouched() and not lab.untouched()


# ---- Python API ------------------------------------------------------------------------------

GOLD = os.path.join(GOLDEN, "kmeans")


@functools.lru_cache(maxsize=None)
def sklearn_golden():
    with np.load(os.path.join(GOLD, "sklearn.npz")) as z:
        return {key: z[key] for key in z.files}


def assert_matches_sklearn(res, case, n):
    z = sklearn_golden()
    assert np.array_equal(res.labels, z[case + "_labels"]), case
    assert res.n_iter == int(z[case + "_n_iter"]), case
    want = float(z[case + "_inertia"])
    print(case, "inertia rel diff", abs(res.inertia - want) / want)
    assert abs(res.inertia - want) <= n * 2.0 ** -52 * want, case


@pytest.mark.parametrize("name,k,n_init", kmeans_ref.CASES, ids=[f"{c[0]}-k{c[1]}-i{c[2]}" for c in kmeans_ref.CASES])
def test_kmeans_equals_sklearn(name, k, n_init):
    from expecto_amd.cluster_and_viz import kmeans
    X = kmeans_ref.INPUTS[name]()
    for seed in kmeans_ref.SEEDS:
        res = kmeans(X.astype(np.float32) if seed == 1 else X, k, n_init=n_init, seed=seed)
        case = kmeans_ref.case_name(name, k, n_init, seed)
        assert_matches_sklearn(res, case, X.shape[0])
        assert res.labels.dtype == np.int32 and res.centres.shape == (k, X.shape[1])
        if n_init == 1:
            assert np.array_equal(res.seeds, sklearn_golden()[case + "_seeds"]) and res.restart == 0


def test_sweep_equals_single_fits():
    from expecto_amd.cluster_and_viz import kmeans, kmeans_sweep
    X = kmeans_ref.INPUTS["gauss2002"]()
    ks = [197, 2, 30]
    timings = {}
    swept = kmeans_sweep(X, ks, seed=0, timings=timings)
    assert set(timings) == {"seeding_ms", "lloyd_ms"}
    assert all(isinstance(v, float) and np.isfinite(v) and v >= 0 for v in timings.values())
    for k, r in zip(ks, swept):
        if k != 2:
            assert_matches_sklearn(r, kmeans_ref.case_name("gauss2002", k, 1, 0), X.shape[0])
    one = kmeans(X, 30, seed=0)
    r = swept[2]
    assert_bits(r.labels, one.labels, "labels")
    assert_bits(r.centres, one.centres, "centres")
    assert r.inertia == one.inertia and r.n_iter == one.n_iter
    X3 = kmeans_ref.INPUTS["blobs300"]()
    want = kmeans_ref.fit(X3, 7, n_init=3, seed=2)
    got = kmeans(X3, 7, n_init=3, seed=2)
    assert got.restart == want["restart"] and got.inertia == want["inertia"]
    assert_bits(got.labels, want["labels"], "labels")
    assert_bits(got.centres, want["centres"], "centres")
    assert_bits(got.seeds, want["seeds"], "seeds")


def test_api_refusals():
    from expecto_amd.cluster_and_viz import kmeans
    X = np.ones((5, 3))
    X[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        kmeans(X, 2)
    with pytest.raises(ValueError, match="n_clusters"):
        kmeans(np.ones((5, 3)), 6)
    with pytest.raises(ValueError, match="2-D"):
        kmeans(np.ones(5), 1)


# ---- CLI -------------------------------------------------------------------------------------

def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_equals_reference_run(tmp_path, capsys):
    from expecto_amd import cluster_and_viz, predict_by_cluster
    src = tmp_path / "in"
    src.mkdir()
    Xr = kmeans_ref.cli_reduced(kmeans_ref.CLI_MARKS)
    np.save(src / "tf_idf_reduced_100.npy", Xr)
    out = tmp_path / "out"
    argv = [str(src), "--belugaFeatures", FEATURES_TSV, *kmeans_ref.CLI_FLAGS]
    capsys.readouterr()
    cluster_and_viz.main(argv + ["-o", str(out), "--seed", "0"])
    assert capsys.readouterr().out.encode() == read(os.path.join(GOLD, "cli", "stdout.txt"))
    for name in ("all_feature_clusters.tsv", "cluster_sizes.tsv"):
        assert read(out / name) == read(os.path.join(GOLD, "cli", name)), name
    clusters = b"".join(f"== cluster_{i}.tsv\n".encode() + read(out / "clusters" / f"cluster_{i}.tsv") for i in range(30))
    assert clusters == read(os.path.join(GOLD, "cli", "clusters.txt"))
    assert sorted(os.listdir(out / "clusters")) == sorted(f"cluster_{i}.tsv" for i in range(30))
    assert not (out / "elbow.tsv").exists()
    # predict_by_cluster's reader takes the file
    ids, members = predict_by_cluster.feature_clusters(str(out / "all_feature_clusters.tsv"), kmeans_ref.CLI_MARKS)
    assert ids == list(range(30)) and sum(len(m) for m in members) == kmeans_ref.CLI_MARKS
    # --elbow: kmeans_sweep's table beside the same cluster files
    swept = tmp_path / "swept"
    cluster_and_viz.main(argv + ["-o", str(swept), "--elbow", "2", "40", "9", "--n_init", "2", "--n_clusters", "30"])
    ks = list(range(2, 40, 9))
    res = cluster_and_viz.kmeans_sweep(Xr[:, :20], ks, n_init=2, seed=0)
    want = "k\tinertia\tn_iter\trestart\n" + "".join(f"{k}\t{r.inertia!r}\t{r.n_iter}\t{r.restart}\n"
                                                     for k, r in zip(ks, res))
    assert read(swept / "elbow.tsv") == want.encode()
    labels = pd.read_csv(swept / "all_feature_clusters.tsv", sep="\t", index_col=0)["cluster"].to_numpy()
    assert np.array_equal(labels, cluster_and_viz.kmeans(Xr[:, :20], 30, n_init=2, seed=0).labels)
    # other options and the row-count refusal
    cluster_and_viz.main(argv + ["-o", str(tmp_path / "k5"), "--n_clusters", "5", "--n_pcs", "7", "--seed", "3"])
    got = pd.read_csv(tmp_path / "k5" / "all_feature_clusters.tsv", sep="\t", index_col=0)["cluster"].to_numpy()
    assert np.array_equal(got, kmeans_ref.fit(Xr[:, :7].astype(np.float64), 5, seed=3)["labels"])
    with pytest.raises(ValueError, match="334 rows"):
        cluster_and_viz.main([str(src), "--belugaFeatures", FEATURES_TSV, "--no_tf_features", "-o", str(tmp_path / "bad")])
