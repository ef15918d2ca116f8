"""GPU: saturation mutagenesis.  expecto_ism_variants against its numpy restatement; expecto_ism_score
bit for bit against the chain of existing entry points on the same device buffers
(expecto_fwd_rc_average -> expecto_variant_reduce_lut -> expecto_gblinear_predict per model);
expecto_amd.mutagenesis.saturation against the same SNVs through VariantPipeline.predict,
expecto_amd.closest and predict.score_rows; the CLI."""
import math
import os

import numpy as np
import pytest

import ism_ref
from conftest import GOLDEN
from guarded import Guarded, P, ST, assert_bits, dev

pytestmark = pytest.mark.gpu

GENOME_ARGS = dict(n_contigs=3, contig_len=60000, seed=7)   # the synthetic genome of test_gpu_pipelines.py
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from expecto_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------- expecto_ism_variants
def _genome_codes():
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 4, 700).astype(np.uint8)
    codes[100:104] = [0, 1, 2, 3]
    codes[104:111] = 4                                        # a run of non-base codes
    codes[0], codes[-1] = 2, 4
    return codes


@pytest.mark.parametrize("start,L", [(0, 1), (0, 3), (98, 64), (98, 65), (0, 257), (699, 1), (443, 257), (636, 64)])
def test_variants_equal_the_restatement(lib, start, L):
    codes = _genome_codes()
    assert start + L <= codes.size and (start == 0 or start + L == codes.size or (start <= 100 and start + L >= 111))
    g = dev(codes)
    outs = [Guarded((3 * L,), np.int64)] + [Guarded((3 * L,), np.uint8, offset=o) for o in (0, 1, 3)]
    assert lib.expecto_ism_variants(P(g), codes.size, start, L, *(o.ptr for o in outs), ST()) == 0
    for o, want, what in zip(outs, ism_ref.variants(codes, start, L), ("var_off", "ref_code", "alt_code", "valid")):
        assert_bits(o.result(), want, what)


def test_variants_refuse_a_region_outside_the_genome(lib):
    g = dev(_genome_codes())
    outs = [Guarded((9,), np.int64)] + [Guarded((9,), np.uint8) for _ in range(3)]
    for start, L in ((-1, 3), (698, 3), (0, -1)):
        assert lib.expecto_ism_variants(P(g), 700, start, L, *(o.ptr for o in outs), ST()) == EINVAL
    assert all(o.untouched() for o in outs)


# ---------------------------------------------------------------------------- expecto_ism_score
SHIFTS = {1: [0], 3: [0, -200, 200], 9: [0, -200, -400, -600, -800, 200, 400, 600, 800]}
POS_DIST = [0, -200, 1234, 200, -777]     # dist + shift hits 0 (both masks fire), negatives and positives


def _case(S, F, M, npos, seed, per_slot_dist=False):
    import torch
    rng = np.random.default_rng(seed)
    n = 3 * npos
    keep = np.sort(rng.choice(F, max(1, F - 1 - F // 5), replace=False)).astype(np.int32)   # nk < F, irregular
    y = rng.normal(0, 1, (2, 2, S, n, F)).astype(np.float32)
    y[:, 0] = np.repeat(y[:, 0, :, 0::3], 3, axis=2)           # the three slots of a position: one ref window
    dist = np.repeat(np.asarray(POS_DIST[:npos], np.int64), 3)
    if per_slot_dist:
        dist = dist + np.tile(np.array([0, 200, -431]), npos)
    w = rng.normal(0, 1, (10 * keep.size, M)).astype(np.float32)
    w[rng.random(w.shape) < 0.2] = 0.0
    init = rng.normal(2, 1, M).astype(np.float32)
    valid = np.ones(n, np.uint8)
    if npos >= 2:
        valid[3:6] = 0                                          # one position entirely invalid, next to valid ones
    if per_slot_dist:
        valid[1] = 0
    shifts = SHIFTS[S]
    reach = int(np.abs(dist).max()) + max(abs(s) for s in shifts)
    lut_len = max(1, reach // 200)                              # the largest fl (= reach // 200) is past the table
    lut = np.stack([np.exp(-c * np.arange(lut_len, dtype=np.float64)) for c in (0.01, 0.02, 0.05, 0.1, 0.2)])
    t = dict(y=dev(y), dist=dev(dist), shifts=dev(np.asarray(shifts, np.int32)), lut=dev(lut), keep=dev(keep),
             w=dev(w), init=dev(init), valid=dev(valid))
    return dict(S=S, F=F, M=M, n=n, nk=keep.size, lut_len=lut_len, host=dict(keep=keep, w=w, init=init, valid=valid,
                                                                              dist=dist), **t), torch


def _chain(lib, c, plus):
    """float32 [2 alleles, M, n]: the existing entry points, one after the other, on the case's buffers."""
    import torch
    S, F, M, n, nk = c["S"], c["F"], c["M"], c["n"], c["nk"]
    cols = dev((np.arange(10, dtype=np.int32)[:, None] * F + c["host"]["keep"][None, :]).reshape(-1).astype(np.int32))
    sp = torch.full((n,), 1 if plus else 0, dtype=torch.uint8, device="cuda")
    out = torch.empty((2, M, n), dtype=torch.float32, device="cuda")
    for a in range(2):
        x = c["y"][:, a].contiguous()                            # [2, S, n, F]: fwd rows then rc rows
        avg = torch.empty((S * n, F), dtype=torch.float32, device="cuda")
        assert lib.expecto_fwd_rc_average(P(x), S * n, F, P(avg), ST()) == 0
        feat = torch.empty((n, 10 * F), dtype=torch.float64, device="cuda")
        assert lib.expecto_variant_reduce_lut(P(avg), P(c["dist"]), P(sp), P(c["shifts"]), S, n, F, P(c["lut"]),
                                              c["lut_len"], P(feat), ST()) == 0
        for m in range(M):
            wm = c["w"][:, m].contiguous()
            assert lib.expecto_gblinear_predict(P(feat), n, 10 * F, P(cols), 10 * nk, P(wm),
                                                float(c["host"]["init"][m]), P(out[a, m]), ST()) == 0
    return out.cpu().numpy()


def _score(lib, c, plus, outs=None, n=None, n_shift=None, nk=None, nfeat=None):
    S, F, M = c["S"], c["F"], c["M"]
    n = c["n"] if n is None else n
    outs = outs or (Guarded((M, n), np.float32, offset=4), Guarded((M, n // 3), np.float32), Guarded((M, n), np.float64))
    st = lib.expecto_ism_score(P(c["y"][0, 0]), P(c["y"][0, 1]), 2 * S * c["n"], P(c["dist"]), int(plus), P(c["shifts"]),
                               S if n_shift is None else n_shift, n, F if nfeat is None else nfeat, P(c["lut"]),
                               c["lut_len"], P(c["keep"]), c["nk"] if nk is None else nk, P(c["w"]), P(c["init"]), M,
                               P(c["valid"]), *(o.ptr for o in outs), ST())
    return st, outs


def _expected(c, ref, alt):
    valid = c["host"]["valid"].astype(bool)
    want_ref = ref[:, 0::3].copy()
    want_sed = alt.astype(np.float64) - np.repeat(want_ref, 3, axis=1).astype(np.float64)
    want_alt = alt.copy()
    want_alt[:, ~valid] = np.nan
    want_sed[:, ~valid] = np.nan
    want_ref[:, ~valid.reshape(-1, 3).any(1)] = np.nan
    return want_alt, want_ref, want_sed


@pytest.mark.parametrize("S,F,M,npos,plus", [(1, 7, 1, 1, True), (1, 70, 3, 2, False), (3, 7, 64, 5, True),
                                             (3, 70, 65, 2, False), (9, 70, 3, 5, True), (9, 2002, 65, 2, False),
                                             (3, 2002, 1, 1, True), (9, 7, 64, 5, False)])
def test_score_equals_the_chain_of_existing_entry_points(lib, S, F, M, npos, plus):
    c, torch = _case(S, F, M, npos, seed=100 * S + F + M)
    ref, alt = _chain(lib, c, plus)
    for m in range(M):      # the chain's REF is one value per position: the three slots hold one ref window
        assert_bits(ref[m, 0::3], ref[m, 1::3], "chain REF, slots 0 and 1")
        assert_bits(ref[m, 0::3], ref[m, 2::3], "chain REF, slots 0 and 2")
    st, outs = _score(lib, c, plus)
    assert st == 0
    got_alt, got_ref, got_sed = (o.result() for o in outs)
    want_alt, want_ref, want_sed = _expected(c, ref, alt)
    assert_bits(got_alt, want_alt, "alt_pred")
    assert_bits(got_ref, want_ref, "ref_pred")
    assert_bits(got_sed, want_sed, "sed")
    assert np.isfinite(got_alt[:, c["host"]["valid"].astype(bool)]).all()
    # the restatement agrees wherever the table covers the distance (numpy's exp is the table's)
    # and the two summaries follow it
    from expecto_amd import mutagenesis as mg
    vp, dr = mg.summaries(torch.from_numpy(got_sed).cuda(), c["valid"])
    want_vp, want_dr = ism_ref.summaries(got_sed, c["host"]["valid"])
    assert_bits(vp.cpu().numpy(), want_vp, "variation_potential")
    assert_bits(dr.cpu().numpy(), want_dr, "directionality")


def test_score_reads_each_slots_own_distance_and_validity(lib):
    """Slots of one position with different distances and one of them invalid: every alt follows the
    chain at its own distance, the position's ref is the chain's REF of its first slot."""
    c, _ = _case(3, 70, 3, 2, seed=9, per_slot_dist=True)
    ref, alt = _chain(lib, c, True)
    st, outs = _score(lib, c, True)
    assert st == 0
    want_alt, want_ref, want_sed = _expected(c, ref, alt)
    for o, want, what in zip(outs, (want_alt, want_ref, want_sed), ("alt_pred", "ref_pred", "sed")):
        assert_bits(o.result(), want, what)
    assert np.isnan(outs[0].result()[:, 1]).all() and np.isfinite(outs[1].result()[:, 0]).all()


def test_summary_orders_are_the_headers(lib):
    import torch
    from expecto_amd import mutagenesis as mg
    rng = np.random.default_rng(5)
    for n in (0, 3, 63, 66, 201):
        sed = rng.normal(0, 1, (3, n)) * 10.0 ** rng.integers(-6, 6, (3, n))
        valid = (rng.random(n) < 0.8).astype(np.uint8)
        sed[:, valid == 0] = np.nan
        vp, dr = mg.summaries(torch.from_numpy(sed).cuda(), torch.from_numpy(valid).cuda())
        want_vp, want_dr = ism_ref.summaries(sed, valid)
        assert_bits(vp.cpu().numpy(), want_vp, f"variation_potential n={n}")
        assert_bits(dr.cpu().numpy(), want_dr, f"directionality n={n}")


@pytest.mark.parametrize("bad", ["n % 3", "nk", "n_shift"])
def test_score_refuses_bad_shapes_and_writes_nothing(lib, bad):
    c, _ = _case(3, 70, 3, 2, seed=1)
    M, n = c["M"], c["n"]
    outs = (Guarded((M, n), np.float32), Guarded((M, n // 3), np.float32), Guarded((M, n), np.float64))
    kw = {"n % 3": dict(n=n - 2), "nk": dict(nk=10241, nfeat=10241), "n_shift": dict(n_shift=820)}[bad]
    st, _ = _score(lib, c, True, outs=outs, **kw)     # nothing is read: the call is refused before any launch
    assert st == EINVAL and lib.expecto_last_error().decode()
    assert all(o.untouched() for o in outs)


# ---------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from expecto_amd import beluga, synthetic
    from expecto_amd.genome import DeviceGenome, Fasta
    from expecto_amd.pipeline import VariantPipeline
    from expecto_amd.xgblinear import GBLinear
    g = synthetic.genome_bytes(**GENOME_ARGS)
    fa = Fasta.from_dict(g)
    eng = beluga.seeded(0, gain=math.sqrt(6.0), max_batch=300).cuda().engine()
    pipe = VariantPipeline(eng, fa, DeviceGenome(fa))
    rng = np.random.default_rng(17)
    keep = np.sort(rng.choice(2002, 1777, replace=False)).astype(np.int32)
    models = []
    for _ in range(2):
        w = rng.normal(0, 0.05, (10 * keep.size, 1)).astype(np.float32)
        w[rng.random(w.shape) < 0.3] = 0.0
        models.append(GBLinear(w, rng.normal(0, 1, 1).astype(np.float32), 2.0))
    # six consecutive positions of chr1 with exactly one N among them
    s = np.frombuffer(g["chr1"], np.uint8)
    isn = (s == ord("N")) | (s == ord("n"))
    cnt = np.convolve(isn.astype(int), np.ones(6, int), "valid")
    first0 = int(np.nonzero((cnt == 1) & (np.arange(cnt.size) > 20000) & ~isn[:cnt.size] & ~isn[5:])[0][0])
    return dict(g=g, fa=fa, pipe=pipe, keep=keep, models=models, first=first0 + 1, dir=tmp_path_factory.mktemp("ism"))


@pytest.mark.parametrize("maxshift", [800, 0])
@pytest.mark.parametrize("strand", ["+", "-"])
def test_saturation_equals_the_explicit_variant_path(world, strand, maxshift):
    import pandas as pd
    import torch
    from expecto_amd import closest, predict
    from expecto_amd import mutagenesis as mg
    from expecto_amd.features import fwd_rc_average
    from expecto_amd.pipeline import VariantSet, shift_order
    pipe, models, keep, first = world["pipe"], world["models"], world["keep"], world["first"]
    tss = first + 3 if strand == "+" else first + 2             # both regions: first .. first + 5
    bank = mg.ModelBank(models, keep)
    res = mg.saturation(pipe, bank, "chr1", tss, strand, upstream=3, downstream=3, maxshift=maxshift,
                        positions_per_batch=4)                  # two batches: 4 and 2 positions
    assert res.pos.tolist() == list(range(first, first + 6)) and res.dist.tolist() == [p - tss for p in res.pos]
    valid = res.valid.cpu().numpy().astype(bool)
    assert valid.sum() == 15 and (valid.reshape(6, 3).all(1) | ~valid.reshape(6, 3).any(1)).all()
    # the same SNVs, written out, through the existing path
    d = world["dir"] / f"{strand == '+'}_{maxshift}"
    os.makedirs(d, exist_ok=True)
    chrom, pos, ref, alt = mg.slot_table("chr1", res.pos, res.ref_base.cpu().numpy(), res.alt_code.cpu().numpy(), valid)
    assert all(chr(world["g"]["chr1"][p - 1]).upper() == r for p, r in zip(pos, ref))
    vs = VariantSet(list(chrom), pos, list(ref), list(alt))
    shifts = shift_order(maxshift)
    y = pipe.predict(vs, shifts)                                 # [2, 2, S, 15, 2002]
    nv, S = len(vs), len(shifts)
    eff = {k: torch.stack([fwd_rc_average(y[:, a, j].reshape(2 * nv, 2002)) for j in range(S)])
           for a, k in enumerate(("ref", "alt"))}
    mg.write_vcf(str(d / "in.vcf"), "chr1", res.pos, res.ref_base.cpu().numpy(), res.alt_code.cpu().numpy(), valid)
    anno = d / "anno.csv"
    anno.write_text("id,symbol,seqnames,strand,TSS,CAGE_representative_TSS,type\n"
                    f"ENSGT0001,G1,chr1,{strand},{tss},{tss},protein_coding\n")
    closest.main([str(d / "in.vcf"), "--geneanno_file", str(anno), "-o", str(d / "closest")])
    args = predict.build_parser().parse_args(["--coorFile_chromatin", str(d / "closest" / "snps_hg19.vcf"), "--geneFile",
                                              str(d / "closest" / "closest_genes.tsv"), "--batchSize", "7"])
    rows = predict.Rows(args, torch.device("cuda"))
    assert rows.n == nv and rows.dist.tolist() == [p - tss for p in pos] and (rows.strand == strand).all()
    ref_x, alt_x = predict.score_rows(args, models, eff, rows, keep, shifts, lambda in_batch: None, torch.device("cuda"))
    sed_x = np.asarray(predict.sed_frame(rows, ref_x[0], alt_x[0])["SED"]), alt_x[1] - ref_x[1]
    got_alt, got_sed = res.alt_pred.cpu().numpy(), res.sed_slots.cpu().numpy()
    got_ref = res.ref_pred.cpu().numpy()
    okpos = valid.reshape(6, 3)[:, 0]
    for m in range(2):
        assert_bits(got_alt[m, valid].astype(np.float64), alt_x[m], f"ALT model {m}")
        assert_bits(np.repeat(got_ref[m], 3)[valid].astype(np.float64), ref_x[m], f"REF model {m}")
        assert_bits(got_sed[m, valid], sed_x[m], f"SED model {m}")
    # NaN exactly in the slots the explicit path cannot express
    assert np.isnan(got_alt[:, ~valid]).all() and np.isnan(got_sed[:, ~valid]).all() and np.isnan(got_ref[:, ~okpos]).all()
    assert np.isfinite(got_ref[:, okpos]).all() and np.abs(got_sed[:, valid]).max() > 0
    sed4, ac, rb = res.sed.cpu().numpy(), res.alt_code.cpu().numpy().reshape(6, 3), res.ref_base.cpu().numpy()
    assert sed4.shape == (2, 6, 4)
    for p in range(6):
        if not okpos[p]:
            assert rb[p] == 4 and np.isnan(sed4[:, p]).all()
            continue
        assert_bits(sed4[:, p, rb[p]], np.zeros(2), "the ref allele")          # +0.0
        for j in range(3):
            assert_bits(sed4[:, p, ac[p, j]], got_sed[:, 3 * p + j], "allele axis")
    # one batch gives the same bits
    one = mg.saturation(pipe, bank, "chr1", tss, strand, upstream=3, downstream=3, maxshift=maxshift)
    assert torch.equal(one.alt_pred.view(torch.int32), res.alt_pred.view(torch.int32))
    assert torch.equal(one.sed_slots.view(torch.int64), res.sed_slots.view(torch.int64))


def test_cli_writes_matrices_summary_and_vcf(world, capsys):
    import pandas as pd
    from expecto_amd import chromatin, h5, predict, synthetic
    from expecto_amd import mutagenesis as mg
    d = world["dir"] / "cli"
    os.makedirs(d, exist_ok=True)
    synthetic.write_fasta(str(d / "hg19.fa"), world["g"])
    feats_path = os.path.join(GOLDEN, "predict_sed", "deepsea_beluga_2002_features.tsv")
    keep = np.nonzero(predict.get_keep_mask(predict.read_features_table(feats_path), False, False, False, False, True))[0]
    assert 0 < keep.size < 2002
    from expecto_amd.xgblinear import GBLinear
    rng = np.random.default_rng(23)
    models = [GBLinear(rng.normal(0, 0.05, (10 * keep.size, 1)).astype(np.float32),
                       rng.normal(0, 1, 1).astype(np.float32), 2.0) for _ in range(2)]
    for i, m in enumerate(models):
        m.save_legacy(str(d / f"tissue{i}.save"))
    (d / "modellist").write_text("ModelName\n" + "".join(f"{d}/tissue{i}.save\n" for i in range(2)))
    tss = world["first"] + 3
    (d / "anno.csv").write_text("id,symbol,seqnames,strand,TSS,CAGE_representative_TSS,type\n"
                                f"ENSGT0001,G1,chr1,+,{tss},{tss},protein_coding\n"
                                "ENSGT0002,G2,chr2,-,29000,29123,protein_coding\n")
    out = d / "out"
    mg.main(["--geneanno", str(d / "anno.csv"), "--genes", "ENSGT0001", "--modelList", str(d / "modellist"),
             "--belugaFeatures", feats_path, "--no_pol2", "--upstream", "3", "--downstream", "3", "--maxshift", "200",
             "-o", str(out), "--vcf-out", "--genome", str(d / "hg19.fa"), "--synthetic-weights", "0", "--max-batch", "300"])
    assert sorted(os.listdir(out)) == ["ENSGT0001.ism.h5", "ENSGT0001.vcf", "summary.tsv"]
    timing = {}
    res = mg.saturation(world["pipe"], mg.ModelBank(models, keep), "chr1", tss, "+", 3, 3, 200, timing=timing)
    assert set(timing) == {"forward_ms", "score_ms"}
    assert all(isinstance(v, float) and np.isfinite(v) and v >= 0 for v in timing.values())
    vp, dr = (x.cpu().numpy() for x in res.summaries())
    tab = pd.read_csv(out / "summary.tsv", sep="\t", float_precision="round_trip")
    assert list(tab.columns) == ["gene", "model", "variation_potential", "directionality"]
    assert list(tab["gene"]) == ["ENSGT0001"] * 2 and list(tab["model"]) == ["tissue0.save", "tissue1.save"]
    assert_bits(tab["variation_potential"].to_numpy(), vp, "variation_potential")
    assert_bits(tab["directionality"].to_numpy(), dr, "directionality")
    got = h5.read(str(out / "ENSGT0001.ism.h5"))
    assert_bits(got["sed"], res.sed.cpu().numpy(), "sed")
    assert_bits(got["ref_pred"], res.ref_pred.cpu().numpy(), "ref_pred")
    assert got["pos"].tolist() == res.pos.tolist() and got["dist"].tolist() == res.dist.tolist()
    assert [x.decode() for x in got["models"]] == ["tissue0.save", "tissue1.save"]
    assert [x.decode() for x in got["gene"]] == ["ENSGT0001", "chr1", str(tss), "+"]
    assert b"".join(got["ref_base"]).decode() == "".join("AGCTN"[c] for c in res.ref_base.cpu().numpy())
    # the VCF round-trips to the slot list
    a = chromatin.build_parser().parse_args([str(out / "ENSGT0001.vcf"), "--output_dir", str(d)])
    vs = chromatin.read_variants(a, write_side_files=False)
    valid = res.valid.cpu().numpy().astype(bool)
    chrom, pos, ref, alt = mg.slot_table("chr1", res.pos, res.ref_base.cpu().numpy(), res.alt_code.cpu().numpy(), valid)
    assert (vs.chrom, vs.pos.tolist(), vs.ref, vs.alt) == (list(chrom), pos.tolist(), list(ref), list(alt))
