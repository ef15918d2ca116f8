"""Segment path, both strands in one chunk list (EXPECTO_SEG_MERGE_STRANDS, default 1): a chunk may
hold (strand, segment) entries of both strands, so every stage is launched once per chunk and not
once per strand per chunk.  Only the launch a row rides in changes: every output equals the
one-chain-per-strand form (knob 0) bit for bit (torch.equal, no tolerance) -- whole chunks, chunk
and FC slice boundaries inside a strand and across the strand boundary, with and without pairs,
single strands -- and the per-window forward of every window in its FC1 role.

Shapes: 3 SNVs (odd) on 200-bp sweeps of 10 shifts (every window holds the SNV: direct FC1), 20
shifts (half of them do: direct FC1 beside copied rows) and 30 shifts (a third: the Karatsuba FC1
with its in-place alt pass); both pool2 phases in each."""
import math

import numpy as np
import pytest
import torch

from conftest import sweep_in_roles

pytestmark = pytest.mark.gpu

SWEEPS = {"alt10": list(range(-1000, 1000, 200)), "mixed20": list(range(-2000, 2000, 200)),
          "karatsuba30": list(range(-3000, 3000, 200))}
MAX_BATCH = 64     # every shape above: all 6 (strand, segment) entries fit in one chunk
_ENGINES = {}


def _engine(max_batch=MAX_BATCH, **env):
    """Seeded handles with the same weights (they share the k-mer tables), one per knob setting."""
    import os
    from expecto_amd import beluga
    key = (max_batch, tuple(sorted(env.items())))
    if key not in _ENGINES:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            m = beluga.seeded(0, gain=math.sqrt(6.0), max_batch=max_batch).cuda()
            _ENGINES[key] = (m, m.engine())
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    return _ENGINES[key][1]


@pytest.fixture(scope="module")
def setup():
    from expecto_amd import synthetic
    from expecto_amd.genome import DeviceGenome, Fasta
    from expecto_amd.pipeline import VariantSet
    g = synthetic.genome_bytes(n_contigs=2, contig_len=150_000, seed=23, repeats=True)
    for name in g:   # an N gap in every contig besides the scattered N bases
        s = bytearray(g[name])
        s[40_000:41_500] = b"N" * 1500
        g[name] = bytes(s)
    fa = Fasta.from_dict(g)
    snv = synthetic.snvs(g, 3, seed=9, margin=10_000)
    vs = VariantSet([s[0] for s in snv], np.array([s[1] for s in snv]), [s[2] for s in snv], [s[3] for s in snv])
    yield fa, DeviceGenome(fa), vs
    _ENGINES.clear()
    _BASE.clear()


def _predict(eng, setup, shifts, **kw):
    from expecto_amd.pipeline import VariantPipeline
    fa, dg, vs = setup
    y = VariantPipeline(eng, fa, dg, **kw).predict(vs, shifts).clone()
    torch.cuda.synchronize()
    return y


_BASE = {}


def _base(setup, name, **kw):
    """The one-chain-per-strand result of a sweep (knob 0), computed once."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _BASE:
        _BASE[key] = _predict(_engine(EXPECTO_SEG_MERGE_STRANDS="0"), setup, SWEEPS[name], **kw)
    return _BASE[key]


def _same(got, want, what):
    assert got.shape == want.shape
    assert torch.equal(got, want), f"{what}: max|diff| {float((got - want).abs().max())}"


def _min_max_batch(L, n_ph=2):
    """The smallest max_batch whose workspace holds one segment of L bases (beluga.hip seg_geo and
    forward_segments' seg_cap: P holds max_batch * 1996 * 320, Q max_batch * 496 * 320 elements)."""
    T1 = L - 7
    S1 = (T1 + 3) // 4 * 4
    P1 = (T1 - 7) // 4
    T3 = P1 - 7
    T4 = T3 - 7
    S5 = T4 // 4
    T5 = S5 - 7
    T6 = T5 - 7
    p = max(S1 * 320, (T3 + 3) // 4 * 4 * 480, n_ph * S5 * 480, n_ph * T6 * 640)
    q = max(P1 * 320, T4 * 480, n_ph * T5 * 640)
    return max(-(-p // (1996 * 320)), -(-q // (496 * 320)), n_ph)


@pytest.mark.parametrize("name", list(SWEEPS))
def test_segment_pairs_both_strands(setup, name):
    got = _predict(_engine(), setup, SWEEPS[name])
    assert got.shape[:2] == (2, 2)
    _same(got, _base(setup, name), name)


@pytest.mark.parametrize("name", ["mixed20", "karatsuba30"])
def test_chunk_boundaries(setup, name):
    """Chunks of two segments' windows: (fwd 0, fwd 1), (fwd 2, rc 0), (rc 1, rc 2) -- the middle
    chunk holds the last fwd and the first rc segment; knob 0 under the same cap ends a chunk at the
    strand boundary."""
    cap = str(2 * len(SWEEPS[name]))
    _same(_predict(_engine(EXPECTO_SEG_CHUNK_WINDOWS=cap), setup, SWEEPS[name]), _base(setup, name), "merged, capped")
    _same(_predict(_engine(EXPECTO_SEG_CHUNK_WINDOWS=cap, EXPECTO_SEG_MERGE_STRANDS="0"), setup, SWEEPS[name]),
          _base(setup, name), "per strand, capped")


@pytest.mark.parametrize("name,mb", [("mixed20", 0), ("karatsuba30", 0), ("mixed20", 40), ("karatsuba30", 40)])
def test_fc_slice_boundaries(setup, name, mb):
    """Small max_batch: the smallest the segment length admits (mb 0; a chunk is then one entry), and
    40, where all six entries still fit in one chunk.  FC1 slices are max_batch windows
    (EXPECTO_FC1K_SLICE=1 drops the Karatsuba FC1's larger slice to that), fewer than one strand's,
    so slices end inside a strand and across the strand boundary and the alt pass runs in several."""
    shifts = SWEEPS[name]
    mb = mb or _min_max_batch(2000 + max(shifts) - min(shifts))
    assert mb < 3 * len(shifts)
    got = _predict(_engine(mb, EXPECTO_FC1K_SLICE="1"), setup, shifts)
    want = _predict(_engine(mb, EXPECTO_FC1K_SLICE="1", EXPECTO_SEG_MERGE_STRANDS="0"), setup, shifts)
    _same(got, want, f"max_batch {mb}")
    _same(got, _base(setup, name), f"max_batch {mb} vs {MAX_BATCH}")


def _segments(setup, shifts, n_seg):
    """Segment tables of the first n_seg variants' sweeps, as VariantPipeline lays them out."""
    from expecto_amd import _lib
    from expecto_amd.pipeline import VariantPipeline, gather_segments
    fa, dg, vs = setup
    pipe = VariantPipeline(_engine(), fa, dg)
    seg = pipe.prepare(vs.slice(0, n_seg), shifts)["seg"]
    codes = gather_segments(_lib.load(), dg, seg["start"], seg["L"], seg["splice_pos"], seg["splice_code"])
    return seg, codes


def test_forward_segments_no_pairs(setup):
    from expecto_amd import _lib
    seg, codes = _segments(setup, SWEEPS["mixed20"], 2)
    ys = [_engine(**env).forward_segments(codes, seg["L"], seg["win_seg"], seg["win_off"], seg["win_row"],
                                          _lib.STRAND_BOTH).clone()
          for env in ({}, {"EXPECTO_SEG_MERGE_STRANDS": "0"})]
    assert ys[0].shape[0] == 2 * len(seg["win_seg"])
    _same(ys[0], ys[1], "forward_segments")


@pytest.mark.parametrize("name", ["mixed20", "karatsuba30"])
def test_single_strands(setup, name):
    """STRAND_FWD and STRAND_RC calls (one strand: nothing to merge) give the matching half of a
    STRAND_BOTH call at knob 0."""
    from expecto_amd import _lib
    seg, codes = _segments(setup, SWEEPS[name], 3)
    n = len(seg["win_seg"])

    def run(eng, mode):
        y = torch.zeros((2 if mode == _lib.STRAND_BOTH else 1, 2, n, 2002), device=codes.device)
        yf = y.view(-1, 2002)
        eng.forward_segment_pairs(codes, seg["L"], seg["var_pos"], seg["alt_code"], seg["win_seg"], seg["win_off"],
                                  seg["win_row"], yf, yf[n:], 2 * n, mode)
        torch.cuda.synchronize()
        return y

    both = run(_engine(EXPECTO_SEG_MERGE_STRANDS="0"), _lib.STRAND_BOTH)
    for eng in (_engine(), _engine(EXPECTO_SEG_MERGE_STRANDS="0")):
        _same(run(eng, _lib.STRAND_FWD)[0], both[0], "fwd")
        _same(run(eng, _lib.STRAND_RC)[0], both[1], "rc")
    _same(run(_engine(), _lib.STRAND_BOTH), both, "both")


@pytest.mark.parametrize("name", ["alt10", "karatsuba30"])
def test_windows_in_their_roles(setup, name):
    """One variant: every window of the merged path, on both strands, equals the per-window forward
    of that window in the FC1 role of its own strand's offset (pipeline.fc1_role)."""
    from expecto_amd.pipeline import VariantPipeline
    fa, dg, vs = setup
    one = (fa, dg, vs.slice(1, 2))
    eng = _engine()
    got = _predict(eng, one, SWEEPS[name])
    pipe = VariantPipeline(eng, fa, dg, use_segments=False, use_pairs=False)
    want = sweep_in_roles(eng, lambda: pipe.predict(one[2], SWEEPS[name]), SWEEPS[name])
    for s in range(2):
        _same(got[s], want[s], f"strand {s}")


def test_launch_counts_halve(setup):
    """One chunk either way (per strand at knob 0): with both strands in it, conv3 .. conv6 and FC1
    are launched half as often for the same multiply-adds."""
    stats = {}
    for knob in ("1", "0"):
        eng = _engine(EXPECTO_SEG_MERGE_STRANDS=knob)
        _predict(eng, setup, SWEEPS["karatsuba30"])   # buffers grown, tables built
        eng.set_profiling(True)
        try:
            _predict(eng, setup, SWEEPS["karatsuba30"])
            stats[knob] = eng.layer_times()
        finally:
            eng.set_profiling(False)
    for layer in ("conv3", "conv4", "conv5", "conv6", "fc1"):
        (_, calls1, macs1), (_, calls0, macs0) = stats["1"][layer], stats["0"][layer]
        print(layer, calls1, calls0, macs1, macs0)
        assert calls1 > 0 and 2 * calls1 == calls0, (layer, calls1, calls0)
        assert macs1 == macs0, (layer, macs1, macs0)


@pytest.mark.parametrize("name,mb", [("mixed20", 128), ("karatsuba30", 96)])
def test_no_allocation_in_the_forward(setup, name, mb):
    """A fresh handle's device memory is the same after the first and the third call of one shape."""
    eng = _engine(max_batch=mb)
    sizes = []
    for _ in range(3):
        _predict(eng, setup, SWEEPS[name])
        sizes.append(eng.device_bytes())
    assert sizes[0] == sizes[2], sizes
