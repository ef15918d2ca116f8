"""In-silico saturation mutagenesis around a TSS: every base of a promoter region mutated to the
three other bases, and the predicted expression change of each mutation for every tissue model.

    python -m expecto_amd.mutagenesis --geneanno resources/geneanno.csv --genes ENSG00000134243 \\
        --modelList resources/modellist --belugaFeatures resources/deepsea_beluga_2002_features.tsv \\
        [--no_tf_features ...] [--upstream 1000] [--downstream 1000] [--maxshift 800] -o OUT [--vcf-out]

The reference has no script for this; its route is a VCF of 3 L SNVs per gene through
``chromatin.py``, ``make_closest_genes_file.py`` and ``predict.py`` once per model.  Here nothing is
walked per variant and no ``[n, 20020]`` float64 feature matrix exists:

1. ``expecto_ism_variants`` enumerates the region's SNVs from the device genome: three slots per
   position, slot ``3*p + j`` holding the j-th base code (0=A 1=G 2=C 3=T) that is not the genome's;
   a position that is not a base (N) keeps three no-op slots marked invalid;
2. the ref and alt chromatin rows come from ``VariantPipeline.predict`` on tables built from those
   device arrays (``region_prep``): the SNV segment path with alt-cone reuse, the engine's f16x3
   overflow check and bf16x6 recompute included (the engine's default, non-deferred mode);
3. ``expecto_ism_score`` turns the rows into predictions of all models at once -- fwd/rc average,
   exp-decay placement and gblinear scoring fused, bitwise what ``expecto_fwd_rc_average``,
   ``expecto_variant_reduce_lut`` and ``expecto_gblinear_predict`` give one after the other.

So ``IsmResult.sed[m, p, a]`` equals, bit for bit, the ``SED`` column ``expecto_amd.predict`` writes
for the SNV "position p to base a" when that SNV goes through ``expecto_amd.chromatin``,
``expecto_amd.closest`` and ``expecto_amd.predict`` with model m (``--vcf-out`` writes that VCF).

Region and distance.  The region is ``[tss - upstream, tss + downstream)`` for a gene on ``+`` and
its mirror image ``(tss - downstream, tss + upstream]`` on ``-``; positions are reported in
ascending genome order on both strands.  ``dist = pos - tss``: ``expecto_amd.closest`` writes
``tss_pos - snp_pos`` into the last column of the gene file and ``predict.Rows`` negates it
(``dist = -gene.iloc[:, -1]``); the strand sign is applied inside the reduction, as in
``predict.py:87-109``.

Summaries (this project's definitions; no published table is reproduced): per model and gene,
``variation_potential = S(|sed|)`` and ``directionality = S(sed)`` over the 3 L slots in slot
order, in float64 on the device (``expecto_ism_summary``); S is the fixed summation order
include/expecto_hip.h defines for ``expecto_variant_contrib``, and invalid slots add nothing.
"""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .features import decay_table
from .pipeline import shift_order, to_device

NFEAT = 2002
BASES = "AGCT"                      # base of code 0..3 (encode._LUT)
_CODE_CHARS = np.frombuffer(b"AGCTN", np.uint8)


class ModelBank:
    """gblinear models sharing one keep set, resident on the device in ``expecto_ism_score``'s
    layout: ``w`` float32 ``[10*nk, M]`` (feature column major, so the models of a wave read one
    contiguous run per column), ``init`` float32 ``[M]`` = float32(bias) + float32(base_score)."""

    def __init__(self, models, keep_idx, names=None, device=None):
        models = list(models)
        keep = np.ascontiguousarray(keep_idx, np.int32).reshape(-1)
        if not models:
            raise ValueError("ModelBank: no models")
        if keep.size == 0 or keep.min() < 0 or keep.max() >= NFEAT or np.any(np.diff(keep) <= 0):
            raise ValueError("ModelBank: keep_idx must be ascending mark columns in 0..2001")
        for m in models:
            if m.num_feature != 10 * keep.size or m.groups != 1:
                raise ValueError(f"model has {m.num_feature} features in {m.groups} groups, the keep mask gives "
                                 f"10 x {keep.size} in one")
        self.models, self.keep_idx = models, keep
        self.names = list(names) if names is not None else [f"model{i}" for i in range(len(models))]
        dev = _lib.device_of(device)
        w = np.stack([m.weights[:, 0] for m in models], 1).astype(np.float32)
        init = np.array([np.float32(m.bias[0]) + np.float32(m.base_score) for m in models], np.float32)
        self.w = _lib.upload(w, dev)
        self.init = torch.from_numpy(init).to(dev)
        self.keep = torch.from_numpy(keep).to(dev)

    def __len__(self):
        return len(self.models)


@dataclass
class IsmResult:
    """One gene's effect matrix (device tensors unless noted).  ``sed`` float64 ``[M, L, 4]``: allele
    axis in base-code order (A, G, C, T), +0.0 at the ref allele, NaN at positions that are not a
    base; ``ref_pred`` float32 ``[M, L]``; ``ref_base`` uint8 ``[L]`` codes (4 = not a base); ``pos``
    (1-based) and ``dist`` int64 ``[L]`` host arrays.  Slot level, slot ``3*p + j``: ``alt_pred``
    float32 and ``sed_slots`` float64 ``[M, 3L]``, ``alt_code`` and ``valid`` uint8 ``[3L]``."""
    sed: torch.Tensor
    ref_pred: torch.Tensor
    ref_base: torch.Tensor
    pos: np.ndarray
    dist: np.ndarray
    alt_pred: torch.Tensor
    sed_slots: torch.Tensor
    alt_code: torch.Tensor
    valid: torch.Tensor
    chrom: str = ""
    tss: int = 0
    strand: str = "+"

    def summaries(self):
        """(variation_potential, directionality): float64 ``[M]`` device tensors."""
        return summaries(self.sed_slots, self.valid)


def enumerate_region(dg, start: int, L: int):
    """The 3 L SNV slots of the flat genome offsets ``start .. start + L - 1`` (device tensors
    ``var_off`` int64, ``ref_code``, ``alt_code``, ``valid`` uint8): ``expecto_ism_variants``."""
    dev = dg.codes.device
    var_off = torch.empty(3 * L, dtype=torch.int64, device=dev)
    ref_code, alt_code, valid = (torch.empty(3 * L, dtype=torch.uint8, device=dev) for _ in range(3))
    _lib.call("expecto_ism_variants", _lib.dptr(dg.codes), dg.codes.numel(), int(start), int(L), _lib.dptr(var_off),
              _lib.dptr(ref_code), _lib.dptr(alt_code), _lib.dptr(valid), what="ism_variants")
    return var_off, ref_code, alt_code, valid


def region_prep(pipeline, var_off: torch.Tensor, ref_code: torch.Tensor, alt_code: torch.Tensor, shifts) -> dict:
    """The tables ``VariantPipeline.predict`` takes (what ``prepare`` builds from a VariantSet with
    rows="shift"), from the device arrays of ``enumerate_region``: every slot is an SNV, nothing is
    read back and nothing is walked per variant.  Span and character checks are the caller's, once
    for the region."""
    shifts = list(shifts)
    n, S = int(var_off.numel()), len(shifts)
    dev = var_off.device
    lo_s, hi_s = min(shifts), max(shifts)
    prep = {"n": n, "S": S, "shifts": shifts, "rows": "shift", "snv_idx": torch.arange(n, device=dev),
            "ind_idx": torch.empty(0, dtype=torch.int64, device=dev), "n_snv": n, "n_ind": 0,
            "seg": None, "win": None, "ind_codes": None}
    if n and S > 1 and pipeline.use_segments and all((x - lo_s) % 4 == 0 for x in shifts):
        if not pipeline.use_pairs:
            raise ValueError("saturation mutagenesis runs the segment-pair path (use_pairs=True)")
        v_i, j_i = np.meshgrid(np.arange(n), np.arange(S), indexing="ij")
        prep["seg"] = {
            "L": 2000 + hi_s - lo_s, "pairs": True,
            "start": var_off + (lo_s - 999),
            "splice_pos": torch.full((n,), 999 - lo_s, dtype=torch.int32, device=dev),
            "splice_code": ref_code,
            "alt_code": alt_code,
            "var_pos": np.full(n, 999 - lo_s, np.int32),
            "win_seg": v_i.ravel().astype(np.int32),
            "win_off": (np.asarray(shifts)[j_i.ravel()] - lo_s).astype(np.int32),
            "win_row": (j_i * n + v_i).ravel().astype(np.int32),
        }
    elif n:
        prep["win"] = {"off": var_off, "rc": ref_code, "ac": alt_code,
                       "sh": to_device(np.asarray(shifts, np.int32), dev)}
    return prep


def score_slots(y: torch.Tensor, dist: torch.Tensor, strand_plus: bool, shifts: torch.Tensor, lut: torch.Tensor,
                bank: ModelBank, valid: torch.Tensor, out=None):
    """``expecto_ism_score`` on a prediction ``y[2 strands, 2 alleles, S, n, 2002]`` of n = 3 x
    positions slots: (alt_pred f32 [M, n], ref_pred f32 [M, n/3], sed f64 [M, n])."""
    _, _, S, n, F = y.shape
    M, dev = len(bank), y.device
    if not y.is_contiguous() or y.dtype != torch.float32:
        raise RuntimeError("score_slots: y must be a contiguous fp32 [2, 2, S, n, F] tensor")
    if out is None:
        out = (torch.empty((M, n), dtype=torch.float32, device=dev),
               torch.empty((M, n // 3), dtype=torch.float32, device=dev),
               torch.empty((M, n), dtype=torch.float64, device=dev))
    alt_pred, ref_pred, sed = out
    _lib.call(
        "expecto_ism_score", _lib.dptr(y[0, 0]), _lib.dptr(y[0, 1]), 2 * S * n, _lib.dptr(dist), int(bool(strand_plus)),
        _lib.dptr(shifts), S, n, F, _lib.dptr(lut), int(lut.shape[1]), _lib.dptr(bank.keep), int(bank.keep.numel()),
        _lib.dptr(bank.w), _lib.dptr(bank.init), M, _lib.dptr(valid), _lib.dptr(alt_pred), _lib.dptr(ref_pred),
        _lib.dptr(sed), what="ism_score")
    return out


def summaries(sed_slots: torch.Tensor, valid: torch.Tensor):
    """(S(|sed|), S(sed)) per model over the slots in slot order: ``expecto_ism_summary``."""
    M, n = sed_slots.shape
    out = torch.empty((2, M), dtype=torch.float64, device=sed_slots.device)
    _lib.call("expecto_ism_summary", _lib.dptr(sed_slots.contiguous()), _lib.dptr(valid), M, n, _lib.dptr(out[0]),
              _lib.dptr(out[1]), what="ism_summary")
    return out[0], out[1]


def region_bounds(tss: int, strand_plus: bool, upstream: int, downstream: int):
    """(first 1-based position, length) of the region: [tss - upstream, tss + downstream) on '+',
    its mirror image (tss - downstream, tss + upstream] on '-'."""
    first = tss - upstream if strand_plus else tss - downstream + 1
    return int(first), int(upstream + downstream)


def _strand_plus(strand) -> bool:
    if strand in ("+", 1, True):
        return True
    if strand in ("-", -1, False):
        return False
    raise ValueError(f"strand must be '+' or '-', not {strand!r}")


def _check_region(pipeline, chrom, start, L, shifts):
    """Once for the region's outer span: no window may reach past the contig's guard
    (``check_spans``) or touch a character encodeSeqs rejects (KeyError, as the variant path)."""
    dg = pipeline.dg
    lo, hi = start + min(shifts) - 999, start + L - 1 + max(shifts) + 1000
    dg.check_spans([chrom], [lo], [hi])
    bad = dg.host.invalid_offsets
    if bad.size:
        i = int(np.searchsorted(bad, lo))
        if i < bad.size and bad[i] <= hi:
            raise KeyError(chr(dg.host.invalid_chars[i]))


def saturation(pipeline, models: ModelBank, chrom: str, tss: int, strand, upstream: int = 1000,
               downstream: int = 1000, maxshift: int = 800, positions_per_batch: int = 512,
               timing: dict | None = None) -> IsmResult:
    """Effect matrix of every SNV of the region around ``tss`` (1-based) of a gene on ``chrom`` /
    ``strand`` for the models of a ``ModelBank`` (module docstring).  ``pipeline``: a
    ``VariantPipeline`` (device genome + engine).  The forward runs ``positions_per_batch``
    positions (three SNV segments each) at a time; results do not depend on it.  ``timing``: a dict
    that receives the device milliseconds of the forward and of the scoring (two syncs)."""
    plus = _strand_plus(strand)
    tss = int(tss)
    if upstream < 0 or downstream < 0 or upstream + downstream <= 0 or positions_per_batch <= 0:
        raise ValueError("saturation: upstream + downstream must be positive")
    first, L = region_bounds(tss, plus, int(upstream), int(downstream))
    dg = pipeline.dg
    if first < 1 or first + L - 1 > dg.lengths[chrom]:
        raise ValueError(f"region {chrom}:{first}-{first + L - 1} reaches outside the contig")
    shifts = shift_order(int(maxshift))
    start = dg.offset(chrom, first)
    _check_region(pipeline, chrom, start, L, shifts)
    dev = pipeline.device
    M, n = len(models), 3 * L
    pos = np.arange(first, first + L, dtype=np.int64)
    dist = pos - tss
    var_off, ref_code, alt_code, valid = enumerate_region(dg, start, L)
    dist_d = to_device(dist, dev).repeat_interleave(3)
    shifts_d = to_device(np.asarray(shifts, np.int32), dev)
    lut = to_device(decay_table(dist, np.full(L, plus), shifts), dev)
    alt_pred = torch.empty((M, n), dtype=torch.float32, device=dev)
    ref_pred = torch.empty((M, L), dtype=torch.float32, device=dev)
    sed = torch.empty((M, n), dtype=torch.float64, device=dev)
    ms = {"forward_ms": 0.0, "score_ms": 0.0} if timing is not None else None     # summed over the batches
    for p0 in range(0, L, positions_per_batch):
        p1 = min(L, p0 + positions_per_batch)
        a, b = 3 * p0, 3 * p1
        whole = p0 == 0 and p1 == L
        timer = _lib.EventTimer(ms)
        timer.mark()
        y = pipeline.predict(region_prep(pipeline, var_off[a:b], ref_code[a:b], alt_code[a:b], shifts))
        timer.mark()
        out = score_slots(y, dist_d[a:b], plus, shifts_d, lut, models, valid[a:b],
                          (alt_pred, ref_pred, sed) if whole else None)
        if not whole:                      # the kernel's rows are m * (b - a) + v
            alt_pred[:, a:b], ref_pred[:, p0:p1], sed[:, a:b] = out
        timer.mark(sync=True)
        timer.add("forward_ms", 0)
        timer.add("score_ms", 1)
    if timing is not None:
        timing.update(ms)
    # [M, L, 4] in base-code order: the three alts scattered to their codes, +0.0 at the ref allele
    ok = valid.view(L, 3)[:, 0].bool()
    idx = torch.where(valid.bool(), alt_code, torch.arange(3, device=dev, dtype=torch.uint8).repeat(L)).long()
    sed4 = torch.zeros((M, L, 4), dtype=torch.float64, device=dev)
    sed4.scatter_(2, idx.view(1, L, 3).expand(M, L, 3), sed.view(M, L, 3))
    sed4[:, ~ok] = float("nan")
    return IsmResult(sed4, ref_pred, ref_code.view(L, 3)[:, 0].contiguous(), pos, dist, alt_pred, sed, alt_code, valid,
                     chrom, tss, "+" if plus else "-")


# ---------------------------------------------------------------------------- files
def slot_table(chrom: str, pos, ref_base, alt_code, valid):
    """The valid slots in slot order as (chrom, pos, ref letter, alt letter) columns (host arrays:
    pos [L], ref_base [L] codes, alt_code / valid [3L])."""
    pos, ref_base = np.asarray(pos, np.int64), np.asarray(ref_base, np.uint8)
    alt_code, valid = np.asarray(alt_code, np.uint8), np.asarray(valid, bool)
    keep = np.nonzero(valid)[0]
    p = keep // 3
    ref = _CODE_CHARS[np.minimum(ref_base[p], 4)].view("S1").astype(str)
    alt = _CODE_CHARS[np.minimum(alt_code[keep], 4)].view("S1").astype(str)
    return np.full(keep.size, chrom, dtype=object), pos[p], ref, alt


def write_vcf(path: str, chrom: str, pos, ref_base, alt_code, valid) -> int:
    """The explicit SNV list of a region, valid slots in slot order: the VCF that takes the same
    matrix through ``chromatin`` + ``closest`` + ``predict``.  Returns the number of rows."""
    import pandas as pd
    c, p, ref, alt = slot_table(chrom, pos, ref_base, alt_code, valid)
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\n")
    pd.DataFrame({"c": c, "p": p, "id": ".", "r": ref, "a": alt}).to_csv(path, sep="\t", header=False, index=False,
                                                                      mode="a")
    return int(p.size)


def write_result(path: str, res: IsmResult, names, gene_id: str) -> None:
    """``<gene>.ism.h5``: sed, ref_pred, ref_base (letters), pos, dist (float64: the writer holds
    floats and byte strings), the model names and the gene record."""
    from . import h5
    base = _CODE_CHARS[np.minimum(res.ref_base.cpu().numpy(), 4)].view("S1")
    h5.write(path, {
        "sed": res.sed.cpu().numpy(), "ref_pred": res.ref_pred.cpu().numpy(), "ref_base": base,
        "pos": res.pos.astype(np.float64), "dist": res.dist.astype(np.float64),
        "models": np.array([str(x).encode() for x in names]),
        "gene": np.array([str(x).encode() for x in (gene_id, res.chrom, res.tss, res.strand)])})


# ---------------------------------------------------------------------------- CLI
def build_parser():
    p = argparse.ArgumentParser(description="In-silico saturation mutagenesis around gene TSSs")
    p.add_argument("--geneanno", default="./resources/geneanno.csv",
                   help="gene annotation (id, symbol, seqnames, strand, TSS, CAGE_representative_TSS, type)")
    p.add_argument("--genes", default=None, help="comma-separated gene ids (the annotation's index)")
    p.add_argument("--gene-file", default=None, dest="gene_file", help="file with one gene id per line")
    p.add_argument("--modelList", default="./resources/modellist", dest="modelList",
                   help="tab-separated table with a ModelName column of model files (or one path per line)")
    p.add_argument("--belugaFeatures", dest="belugaFeatures", help="tsv file denoting Beluga features")
    for flag in ("no_tf_features", "no_dnase_features", "no_histone_features", "intersect_with_lambert", "no_pol2"):
        p.add_argument("--" + flag, action="store_true", dest=flag, default=False)
    p.add_argument("--upstream", type=int, default=1000)
    p.add_argument("--downstream", type=int, default=1000)
    p.add_argument("--maxshift", type=int, default=800)
    p.add_argument("-o", dest="out_dir", default="mutagenesis_out")
    p.add_argument("--vcf-out", action="store_true", dest="vcf_out",
                   help="also write <gene>.vcf, the explicit SNV list in slot order")
    p.add_argument("--positions-per-batch", type=int, default=512, dest="positions_per_batch")
    p.add_argument("--genome", default="./resources/hg19.fa")
    p.add_argument("--weights", default="./resources/deepsea.beluga.pth")
    p.add_argument("--synthetic-weights", type=int, default=None, dest="synthetic_weights")
    p.add_argument("--max-batch", type=int, default=8192, dest="max_batch")
    p.add_argument("--base_score", type=float, default=None, help=argparse.SUPPRESS)
    return p


def read_model_list(path: str) -> list:
    """Model file paths of a modelList: the ``ModelName`` column of a tab-separated table, or one
    path per line."""
    lines = [l.strip() for l in open(path).read().splitlines() if l.strip() and not l.startswith("#")]
    if lines and "ModelName" in lines[0].split("\t"):
        col = lines[0].split("\t").index("ModelName")
        return [l.split("\t")[col].strip() for l in lines[1:]]
    return [l.split("\t")[0] for l in lines]


def gene_ids(args, anno) -> list:
    if args.genes and args.gene_file:
        raise ValueError("give --genes or --gene-file, not both")
    if args.genes:
        ids = [g for g in args.genes.split(",") if g]
    elif args.gene_file:
        ids = [l.strip() for l in open(args.gene_file).read().splitlines() if l.strip()]
    else:
        ids = list(anno.index)
    missing = [g for g in ids if g not in anno.index]
    if missing:
        raise KeyError(f"genes not in the annotation: {missing[:5]}")
    return ids


def run(args) -> list:
    import pandas as pd

    from . import chromatin, dist as edist, predict
    from .genome import DeviceGenome, Fasta
    from .pipeline import VariantPipeline
    from .xgblinear import GBLinear

    rank, world, local = edist.init()
    if world > 1:
        torch.cuda.set_device(edist.local_device(local))
    os.makedirs(args.out_dir, exist_ok=True)
    anno = pd.read_csv(args.geneanno, index_col=0)
    anno = anno[~anno.index.duplicated(keep="first")]
    ids = gene_ids(args, anno)
    feats = predict.read_features_table(args.belugaFeatures)
    keep_idx = np.nonzero(predict.get_keep_mask(feats, *predict.mask_arguments(args)))[0].astype(np.int32)
    paths = read_model_list(args.modelList)
    names = [os.path.basename(p) for p in paths]
    bank = ModelBank([GBLinear.load(p, base_score=args.base_score) for p in paths], keep_idx, names)
    fasta = Fasta(args.genome)
    model = chromatin.load_model(args)
    pipe = VariantPipeline(model.engine(), fasta, DeviceGenome(fasta, device="cuda"))
    lo, hi = edist.shard_range(len(ids), rank, world)      # contiguous gene ranges per rank
    rows = []
    for g in ids[lo:hi]:
        rec = anno.loc[g]
        res = saturation(pipe, bank, str(rec["seqnames"]), int(rec["CAGE_representative_TSS"]), str(rec["strand"]),
                         args.upstream, args.downstream, args.maxshift, args.positions_per_batch)
        vp, dr = (x.cpu().numpy() for x in res.summaries())
        write_result(os.path.join(args.out_dir, f"{g}.ism.h5"), res, names, g)
        if args.vcf_out:
            write_vcf(os.path.join(args.out_dir, f"{g}.vcf"), res.chrom, res.pos, res.ref_base.cpu().numpy(),
                      res.alt_code.cpu().numpy(), res.valid.cpu().numpy())
        rows += [(g, names[m], repr(float(vp[m])), repr(float(dr[m]))) for m in range(len(bank))]
    if world > 1:
        import torch.distributed as tdist
        parts = [None] * world
        tdist.all_gather_object(parts, rows)
        rows = [r for part in parts for r in part]
    if rank == 0:
        with open(os.path.join(args.out_dir, "summary.tsv"), "w") as f:
            f.write("gene\tmodel\tvariation_potential\tdirectionality\n")
            f.writelines("\t".join(r) + "\n" for r in rows)
    return rows


def main(argv=None):
    args = build_parser().parse_args(argv)
    _lib.require_gpu("mutagenesis")
    return run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
