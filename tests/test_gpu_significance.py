"""GPU: expecto_amd.significance -- the background (build, save, load), the scoring API against a
closed-form count, and the command line end to end on synthetic ``.diff.h5`` files against the numpy
restatement (tests/ecdf_ref.py) applied to the same files."""
import os

import numpy as np
import pytest

import ecdf_ref
from conftest import GOLDEN
from guarded import assert_bits

pytestmark = pytest.mark.gpu

FEATURES = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
NFEAT = 2002


def _effects(B, C, seed):
    rng = np.random.default_rng(seed)
    E = (rng.normal(0, 0.02, (B, C)) * 10.0 ** rng.integers(-3, 1, (1, C))).astype(np.float32)
    E[rng.random((B, C)) < 0.1] = 0.0                            # ties at zero, of either sign
    E[::7] *= -1
    k = B // 6
    E[k:2 * k, : C // 2] = E[3 * k:4 * k, : C // 2]              # and runs of equal magnitudes
    return E


def test_background_round_trip(tmp_path):
    import torch
    from expecto_amd import significance as sg
    E = _effects(257, 300, seed=1)                               # more marks than one sort block
    assert 300 > sg.SORT_BLOCK
    bg = sg.build_background(torch.from_numpy(E).cuda(), [f"f{i}" for i in range(300)])
    assert (bg.C, bg.n) == (300, 257)
    assert_bits(bg.sorted.cpu().numpy(), np.ascontiguousarray(np.sort(np.abs(E), axis=0).T), "sorted")
    path = str(tmp_path / "background.h5")
    bg.save(path)
    from expecto_amd import h5
    raw = h5.read(path)
    assert sorted(raw) == ["features", "n", "sorted"] and raw["sorted"].dtype == np.float32 and int(raw["n"]) == 257
    back = sg.Background.load(path)
    assert torch.equal(back.sorted.view(torch.int32), bg.sorted.view(torch.int32))
    assert back.features == bg.features == [f"f{i}".encode() for i in range(300)] and back.n == 257
    bad = E.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        sg.build_background(torch.from_numpy(bad).cuda())
    with pytest.raises(ValueError, match="float32"):
        sg.build_background(torch.from_numpy(E))                 # a host tensor: there is no CPU path


def test_background_scored_against_itself():
    """ge[b, c] = B - #{values of column c strictly below |E[b, c]|}, counted by brute force."""
    import torch
    from expecto_amd import significance as sg
    B, C = 300, 50
    E = _effects(B, C, seed=2)
    x = torch.from_numpy(E).cuda()
    bg = sg.build_background(x)
    A = np.abs(E)
    below = (A[None, :, :] < A[:, None, :]).sum(1)               # [b, c]: how many b' have A[b', c] < A[b, c]
    sig = sg.score(bg, x, alpha=0.05)
    assert_bits(sig.ge.cpu().numpy(), (B - below).astype(np.int32), "ge")
    assert int(sig.ge.min()) >= 1 and sig.B == B                 # every value counts itself
    # a column subset on a strided view gives the same columns
    cols = np.array([0, 3, 17, 49], np.int32)
    wide = torch.full((B, C + 9), float("nan"), device="cuda")
    wide[:, :C] = x
    sub = sg.score(bg, wide[:, : C + 1], cols, alpha=0.05)
    assert_bits(sub.ge.cpu().numpy(), (B - below)[:, cols].astype(np.int32), "ge of a column map")
    want = ecdf_ref.summaries(sub.ge.cpu().numpy(), ecdf_ref.lut(B), ecdf_ref.k_alpha(0.05, B))
    for got, w, what in zip((sub.mean_nlog, sub.max_nlog, sub.top, sub.n_sig), want, ("mean", "max", "top", "n_sig")):
        assert_bits(got.cpu().numpy(), w, what)
    assert_bits(sub.evalues().cpu().numpy(), ecdf_ref.evalues(sub.ge.cpu().numpy(), B), "evalues")
    with pytest.raises(ValueError, match="ascending"):
        sg.score(bg, x, [3, 3])
    with pytest.raises(ValueError, match="columns"):
        sg.score(bg, x[:, :10], [3, 12])


def _write_diff(path, eff_fwd, eff_rc):
    from expecto_amd import h5
    h5.write(path, {"diff": np.concatenate([eff_fwd, eff_rc], 0)})


def _averaged(path):
    from expecto_amd import h5
    d = h5.read(path)["diff"]
    n = d.shape[0] // 2
    return (d[:n] + d[n:]) / np.float32(2)


def test_cli_end_to_end(tmp_path):
    import pandas as pd
    from expecto_amd import h5, predict
    from expecto_amd import significance as sg
    rng = np.random.default_rng(3)
    files = []
    for i, nb in enumerate((180, 120)):                          # the background: 300 variants in two files
        p = str(tmp_path / f"bg.chunk{i}.shift_0.diff.h5")
        _write_diff(p, _effects(nb, NFEAT, 10 + i), _effects(nb, NFEAT, 20 + i))
        files.append(p)
    q = str(tmp_path / "snps.shift_0.diff.h5")
    fwd, rc = _effects(40, NFEAT, 30), _effects(40, NFEAT, 31)
    fwd[7], rc[7] = 0.0, -0.0                                    # a variant with no effect at all
    fwd[9, :] = 10.0                                             # and one beyond the whole background
    rc[9, :] = 10.0
    _write_diff(q, fwd, rc)
    vcf = tmp_path / "snps_hg19.vcf"
    vcf.write_text("##fileformat=VCFv4.3\n" + "".join(
        f"chr{1 + i % 3}\t{1000 + 13 * i}\trs{i}\t{'ACGT'[i % 4]}\t{'CGTA'[i % 4]}\n" for i in range(40)))
    out = tmp_path / "out"
    bg_path = str(tmp_path / "background.h5")
    sg.main(["build", "--snpEffectFile", *files, "--belugaFeatures", FEATURES, "-o", bg_path])
    sg.main(["score", "--background", bg_path, "--snpEffectFile", q, "--coorFile_chromatin", str(vcf),
             "--belugaFeatures", FEATURES, "--no_tf_features", "--alpha", "0.02", "--write-evalues", "-o", str(out)])
    assert sorted(os.listdir(out)) == ["evalues.h5", "significance.tsv"]
    # the restatement on the same files
    feats = predict.read_features_table(FEATURES)
    cols = np.nonzero(predict.get_keep_mask(feats, True, False, False, False, False))[0]
    assert 0 < cols.size < NFEAT
    E = np.concatenate([_averaged(p) for p in files], 0)
    rows = np.ascontiguousarray(np.sort(np.abs(E), axis=0).T)
    B = 300
    assert_bits(h5.read(bg_path)["sorted"], rows, "background.h5")
    ge = ecdf_ref.tail_counts(rows, _averaged(q), cols)
    mean, mx, top, n_sig = ecdf_ref.summaries(ge, ecdf_ref.lut(B), ecdf_ref.k_alpha(0.02, B))
    assert_bits(h5.read(str(out / "evalues.h5"))["evalue"], ecdf_ref.evalues(ge, B), "evalues.h5")
    tab = pd.read_csv(out / "significance.tsv", sep="\t", dtype=str, keep_default_na=False)
    assert list(tab.columns) == ["chrom", "pos", "id", "ref", "alt", "mean_neg_log10_e", "max_neg_log10_e",
                                 "top_feature", "n_significant"]
    assert list(tab["id"]) == [f"rs{i}" for i in range(40)] and list(tab["pos"]) == [str(1000 + 13 * i) for i in range(40)]
    assert_bits(np.array([float(v) for v in tab["mean_neg_log10_e"]]), mean, "mean_neg_log10_e")
    assert_bits(np.array([float(v) for v in tab["max_neg_log10_e"]]), mx, "max_neg_log10_e")
    assert all(v == repr(float(m)) for v, m in zip(tab["mean_neg_log10_e"], mean))
    names = feats["Assay type + assay + cell type"].values[cols]
    assert list(tab["top_feature"]) == [names[t] for t in top]
    assert [int(v) for v in tab["n_significant"]] == n_sig.tolist()
    assert not any(name.startswith("TF/") for name in tab["top_feature"])
    # the two planted variants
    assert n_sig[7] == 0 and (ge[7] == B).all() and mean[7] == 0.0
    assert n_sig[9] == cols.size and (ge[9] == 0).all() and top[9] == 0
    assert mx[9] == -np.log10(1.0 / (B + 1.0))
