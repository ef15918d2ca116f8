"""CPU: the host side of gblinear training -- model formats, the CLI's row selection and
bootstrap weights, and the numpy restatements test_gpu_train.py holds the kernels to."""
import numpy as np
import pandas as pd

from gblinear_ref import make_problem, noise_of

from expecto_amd.xgblinear import GBLinear


def _model(nf=97, seed=0):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((nf, 1)) * 10.0 ** rng.integers(-6, 2, (nf, 1))).astype(np.float32)
    w[3] = 0.0
    return GBLinear(w, np.array([0.37218654], np.float32), 2.0)


def test_save_dump_round_trip(tmp_path):
    m = _model()
    path = str(tmp_path / "m.dump")
    m.save_dump(path)
    text = open(path).read().splitlines()
    assert text[0] == "booster[0]:" and text[1] == "bias:" and text[3] == "weight:"
    assert len(text) == 4 + m.num_feature
    back = GBLinear.load(path, base_score=2.0)
    want = np.array([float("%g" % float(x)) for x in m.weights[:, 0]], np.float32)
    np.testing.assert_array_equal(back.weights[:, 0], want)
    np.testing.assert_array_equal(back.bias, np.array([float("%g" % float(m.bias[0]))], np.float32))
    assert back.base_score == 2.0 and back.num_feature == m.num_feature
    np.testing.assert_allclose(back.weights, m.weights, rtol=5e-6, atol=0)     # %g keeps 6 digits


def test_save_legacy_round_trip_is_bit_equal(tmp_path):
    m = _model(nf=20020, seed=1)
    path = str(tmp_path / "m.save")
    m.save_legacy(path)
    back = GBLinear.load(path)
    assert back.weights.tobytes() == m.weights.tobytes() and back.bias.tobytes() == m.bias.tobytes()
    assert back.base_score == 2.0 and back.objective == "reg:linear"


def _anno(tmp_path):
    """60 genes: seqnames cycle over chr1, chr2, chr8, chrX, chrY, chr3; types cycle over
    protein_coding, lincRNA, rRNA, protein_coding; expression column 2 has a -1 (log of a
    negative: nan) at gene 0 and gene 12, column 1 is positive."""
    chrom = ["chr1", "chr2", "chr8", "chrX", "chrY", "chr3"]
    types = ["protein_coding", "lincRNA", "rRNA", "protein_coding"]
    anno = pd.DataFrame({"id": [f"G{i}" for i in range(60)], "seqnames": [chrom[i % 6] for i in range(60)],
                         "type": [types[i % 4] for i in range(60)]})
    rng = np.random.default_rng(5)
    exp = pd.DataFrame({"id": anno["id"], "tissueA": rng.uniform(0.1, 50, 60), "tissueB": rng.uniform(0.1, 50, 60)})
    exp.loc[[0, 12], "tissueB"] = -1.0
    return anno, exp


def test_row_selection_matches_hand_masks(tmp_path):
    from expecto_amd.train import select_rows

    anno, exp = _anno(tmp_path)
    i = np.arange(60)
    on_train_chrom = np.isin(i % 6, [0, 1, 5])          # chr1, chr2, chr3
    on_test_chrom = i % 6 == 2                          # chr8
    for filt_str, type_ok in (("all", i % 4 != 2), ("pc", np.isin(i % 4, [0, 3])), ("lincRNA", i % 4 == 1)):
        tr, te = select_rows(anno, exp["tissueA"], filt_str, 0.0001)
        np.testing.assert_array_equal(tr, on_train_chrom & type_ok)
        np.testing.assert_array_equal(te, on_test_chrom & type_ok)
    finite = ~np.isin(i, [0, 12])
    tr, te = select_rows(anno, exp["tissueB"], "all", 0.0001)
    np.testing.assert_array_equal(tr, on_train_chrom & (i % 4 != 2) & finite)
    np.testing.assert_array_equal(te, on_test_chrom & (i % 4 != 2) & finite)
    assert tr.sum() > 0 and te.sum() > 0 and not tr[0] and not tr[12]


def test_bootstrap_weights_are_the_draw(tmp_path):
    from expecto_amd.train import bootstrap_weights, select_rows

    anno, exp = _anno(tmp_path)
    tr, _ = select_rows(anno, exp["tissueA"], "all", 0.0001)
    for seed in (0, 7):
        w = bootstrap_weights(tr, seed)
        np.random.seed(seed)                                         # train_bootstrap.py:55, :88-90
        trainind = np.where(tr)[0]
        draw = np.random.choice(trainind, size=trainind.shape[0], replace=True)
        np.testing.assert_array_equal(w, np.bincount(draw, minlength=60))
        assert w.sum() == tr.sum() and (w[~tr] == 0).all()


def test_target_indices():
    from expecto_amd.train import target_indices

    assert target_indices(["1", "2"], 5) == [1, 2]
    assert target_indices(["all"], 5) == [1, 2, 3, 4]


def test_restatements_agree_to_their_noise():
    """R32 and R64 differ (they are not one code path) and by no more than float32 rounding can
    build up: every round adds to a weight one float32-rounded step, whose inputs carry the
    rounding of the F steps before it, so the relative gap is bounded by eps32 * F * rounds."""
    X, y, h = make_problem(1003, 97, seed=11)
    for eta, lam, rounds in ((0.01, 100.0, 5), (0.5, 1.0, 8), (1.0, 0.0, 3)):
        r32, noise, _ = noise_of(X, y, h, eta=eta, lam=lam, rounds=rounds)
        rel = noise[0] / np.abs(r32[0]).max()
        print(f"eta {eta} lambda {lam} rounds {rounds}: noise {noise[0]:.3g}, relative {rel:.3g}")
        assert 0 < rel <= np.finfo(np.float32).eps * 97 * rounds
