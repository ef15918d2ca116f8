"""CPU: the numpy restatement of the saturation-mutagenesis entry points (tests/ism_ref.py) against
hand-written loops, and the host side of expecto_amd.mutagenesis (arguments, region, VCF writer)."""
import numpy as np
import pytest

import ism_ref
from oracle import gblinear_np, reduce_np


def test_enumeration_restatement_equals_a_loop():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 5, 300).astype(np.uint8)
    codes[40:47] = 4
    for start, L in ((0, 1), (0, 300), (37, 65), (299, 1)):
        off, ref, alt, valid = ism_ref.variants(codes, start, L)
        want = [(start + p, codes[start + p], a if codes[start + p] < 4 else codes[start + p], int(codes[start + p] < 4))
                for p in range(L)
                for a in ([b for b in range(4) if b != codes[start + p]] if codes[start + p] < 4 else [4, 4, 4])]
        assert [tuple(int(x) for x in r) for r in zip(off, ref, alt, valid)] == [tuple(int(x) for x in r) for r in want]
        assert off.dtype == np.int64 and ref.dtype == alt.dtype == valid.dtype == np.uint8


def test_score_restatement_equals_the_oracles_composed_by_hand():
    rng = np.random.default_rng(1)
    S, P, F, M = 3, 2, 7, 2
    n, shifts = 3 * P, [0, -200, 200]
    keep = np.array([0, 2, 3, 6])
    y_ref = rng.normal(0, 1, (2, S, n, F)).astype(np.float32)
    y_ref = np.repeat(y_ref[:, :, 0::3], 3, axis=2)
    y_alt = rng.normal(0, 1, (2, S, n, F)).astype(np.float32)
    dist = np.repeat(np.array([-200, 431]), 3)
    w = rng.normal(0, 1, (10 * keep.size, M)).astype(np.float32)
    init = np.array([2.5, -1.0], np.float32)
    valid = np.array([1, 1, 1, 0, 0, 0], np.uint8)
    alt, ref, sed = ism_ref.score(y_ref, y_alt, dist, False, shifts, keep, w, init, valid)
    cols = (np.arange(10)[:, None] * F + keep[None, :]).reshape(-1)
    wts = reduce_np.variant_weights(dist, np.zeros(n, bool), shifts)
    for m in range(M):
        preds = []
        for y in (y_ref, y_alt):
            effs = [reduce_np.fwd_rc_average(np.concatenate([y[0, j], y[1, j]])) for j in range(S)]
            x = reduce_np.variant_reduce(effs, wts, F)
            preds.append(gblinear_np.predict(x[:, cols], w[:, m], init[m], 0.0))
        assert np.array_equal(alt[m, :3], preds[1][:3]) and np.isnan(alt[m, 3:]).all()
        assert ref[m, 0] == preds[0][0] == preds[0][1] == preds[0][2] and np.isnan(ref[m, 1])
        assert np.array_equal(sed[m, :3], preds[1][:3].astype(np.float64) - np.float64(preds[0][0]))
        assert np.isnan(sed[m, 3:]).all()
    assert alt.dtype == ref.dtype == np.float32 and sed.dtype == np.float64


def _header_S(x):
    """include/expecto_hip.h, expecto_variant_contrib: p[l] = x_l + x_{l+64} + ... left to right
    (-0.0 where there is no term), then p[l] += p[l+s] for l < s, s = 32 .. 1; S of nothing is +0.0."""
    if len(x) == 0:
        return 0.0
    p = []
    for l in range(64):
        terms = list(x[l::64])
        acc = -0.0
        for k, t in enumerate(terms):
            acc = t if k == 0 else acc + t
        p.append(np.float64(acc))
    for s in (32, 16, 8, 4, 2, 1):
        for l in range(s):
            p[l] = p[l] + p[l + s]
    return p[0]


@pytest.mark.parametrize("c", [0, 1, 63, 64, 65, 200])
def test_S_follows_the_header(c):
    x = np.random.default_rng(c).normal(0, 1, c) * 10.0 ** np.random.default_rng(c + 1).integers(-8, 8, c)
    got, want = ism_ref.S(x), _header_S(x)
    assert np.float64(got).tobytes() == np.float64(want).tobytes()
    if c == 1:
        assert np.float64(ism_ref.S(np.array([-0.0]))).tobytes() == np.float64(-0.0).tobytes()


def test_summaries_skip_invalid_slots():
    sed = np.array([[1.5, np.nan, -2.25, np.nan, np.nan, np.nan]])
    valid = np.array([1, 0, 1, 0, 0, 0])
    vp, dr = ism_ref.summaries(sed, valid)
    assert vp[0] == 3.75 and dr[0] == -0.75


def test_cli_arguments():
    from expecto_amd import mutagenesis as mg
    a = mg.build_parser().parse_args(["--geneanno", "g.csv", "--genes", "G1,G2", "--modelList", "ml", "--belugaFeatures",
                                      "f.tsv", "--no_tf_features", "--no_pol2", "-o", "out", "--vcf-out"])
    assert (a.upstream, a.downstream, a.maxshift) == (1000, 1000, 800)
    assert a.genes == "G1,G2" and a.gene_file is None and a.vcf_out and a.out_dir == "out"
    from expecto_amd import predict
    assert predict.mask_arguments(a) == (True, False, False, False, True)
    a = mg.build_parser().parse_args(["--gene-file", "ids.txt", "--upstream", "50", "--downstream", "20", "--maxshift", "0"])
    assert (a.gene_file, a.upstream, a.downstream, a.maxshift, a.vcf_out) == ("ids.txt", 50, 20, 0, False)


def test_region_mirrors_on_the_minus_strand(tmp_path):
    from expecto_amd import mutagenesis as mg
    assert mg.region_bounds(1000, True, 10, 4) == (990, 14)        # [990, 1004)
    assert mg.region_bounds(1000, False, 10, 4) == (997, 14)       # (996, 1010]
    ml = tmp_path / "modellist"
    ml.write_text("ModelName\tTissue\n a.save\tliver\nb.save\tlung\n")
    assert mg.read_model_list(str(ml)) == ["a.save", "b.save"]
    ml.write_text("a.save\n\nb.save\n")
    assert mg.read_model_list(str(ml)) == ["a.save", "b.save"]


def test_vcf_writer_lists_the_valid_slots_in_slot_order(tmp_path):
    from expecto_amd import mutagenesis as mg
    codes = np.array([0, 3, 4, 2, 1], np.uint8)                   # A T N C G
    _, ref, alt, valid = ism_ref.variants(codes, 0, 5)
    path = tmp_path / "toy.vcf"
    n = mg.write_vcf(str(path), "chr2", np.arange(101, 106), codes, alt, valid)
    lines = path.read_text().splitlines()
    assert lines[0].startswith("##fileformat=VCF") and lines[1].startswith("#CHROM")
    rows = [tuple(l.split("\t")) for l in lines[2:]]
    want = [("chr2", str(p), ".", r, a) for p, r, alts in
            ((101, "A", "GCT"), (102, "T", "AGC"), (104, "C", "AGT"), (105, "G", "ACT")) for a in alts]
    assert rows == want and n == 12
