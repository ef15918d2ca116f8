"""The segment path (forward_segments, forward_segment_pairs) over the geometry seg_plan accepts and
the other GPU tests do not reach: every count of pool2 phases (1, 2, 3, 4) and two-phase sets other
than {0, 2}, segment lengths of every residue mod 16 (so T4 % 4 = 0, 1, 2, 3: the last pool2 group of
the higher phases hangs over the segment's valid conv4 rows), L = 2000 (one window per segment, every
clamp of the alt runs at its minimum), both strands on disjoint phases, the fused conv4 + pool2
epilogue with T4 % 4 = 1 and 3, SNVs at the segment's and the windows' edges and one that no window
holds, N and the reference base as the alt allele.

Every window, ref and alt, on every computed strand equals forward_codes of the window's own 2000
codes bit for bit (torch.equal; outputs filled with NaN first), in the f16x3 default without one
overflow fallback, and the first and last window of a segment meet the float64 forward at the parity
bar (tests/seg_cases.py).  Three random segments of codes 0..4 per case; the cases and what each
reaches:

  L     offsets         mode  phases        T4 % 4  pool2
  2000  0               fwd   {0}           2       pass    (also rc, both)
  2016  0 16            both  {0}           2       pass
  2008  0 8             both  {0,2}         0       fused
  2004  0 4             both  {0,1}         3       pass
  2012  0 12            both  {0,3}         1       pass
  2204  0 200 204       fwd   {0,2,3}       1       pass
  2204  0 200 204       rc    {0,1,3}       1       pass
  2204  0 200 204       both  {0,1,2,3}     1       pass
  2204  0 204           rc    {0,3}         1       pass
  2212  0 8 200 208     fwd   {0,2}         3       fused
  2212  0 8 200 208     both  {0,1,2,3}     3       pass    (fwd {0,2}, rc {1,3})
  2220  0 200 216       fwd   {0,2}         1       fused
"""
import math
import os

import pytest
import torch

import seg_cases
from seg_cases import BY_ID, CASES, run_case

pytestmark = pytest.mark.gpu

MAX_BATCH = 64
_ENGINES = {}


def _knob_engine(tag="", **env):
    """A fresh seeded handle (same weights) built under the given knobs, kept for the module."""
    from expecto_amd import beluga
    key = (tag, tuple(sorted(env.items())))
    if key not in _ENGINES:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            m = beluga.seeded(0, gain=math.sqrt(6.0), max_batch=MAX_BATCH).cuda()
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
    from expecto_amd import beluga
    m = beluga.seeded(0, gain=math.sqrt(6.0), max_batch=MAX_BATCH)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    eng = m.engine()
    assert eng.precision == "f16x3"
    yield eng, sd
    _ENGINES.clear()
    seg_cases._Y64.clear()


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_every_window_equals_its_own_forward(setup, cid):
    eng, sd = setup
    run_case(eng, sd, BY_ID[cid])


# (case, segments): 3 segments reach the fused epilogue in each (256-row tiles, 7 to 12 of them); the
# segment counts make every case need more seam and edge rows than the one before it
FUSED = [("L2220-0_200_216-fwd", 3), ("L2212-0_8_200_208-fwd", 4), ("L2008-0_8-both", 3)]


def test_fused_epilogue_ran_and_equals_the_pool_pass(setup):
    """The cases listed as fused take conv4's pool2 epilogue: a handle with EXPECTO_POOL_FUSED=0 gives
    the same bits, and only the default handle holds the epilogue's buffers -- 4 unpooled seam rows
    per 256-row tile of the conv4 launch (pool2_tile_seams) and, after a pairs call, kSegEdge = 32 ref
    rows per (strand, segment) entry (seg_delta_pool), of 480 floats; run_conv4_pool_fused alone
    reserves them, and the handle's device bytes count them exactly."""
    _, sd = setup
    assert [BY_ID[c].pool for c, _ in FUSED] == ["fused"] * 3
    assert sorted(c for c, _ in FUSED) == sorted(c.id for c in CASES if c.pool == "fused")
    fused, plain = _knob_engine("fused"), _knob_engine(EXPECTO_POOL_FUSED="0")
    warm = BY_ID["L2004-0_4-both"]          # phases {0, 1}: the pool pass on both handles; tables and buffers grown
    for eng in (fused, plain):
        run_case(eng, sd, warm, ns=4, f64=False)
    base = fused.device_bytes() - plain.device_bytes()
    seam = edge = 0
    for cid, ns in FUSED:
        case = BY_ID[cid]
        a = run_case(fused, sd, case, ns=ns, f64=False)
        b = run_case(plain, sd, case, ns=ns, f64=False)
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), cid
        t3p = ((case.L - 14) // 4 - 7 + 3) & ~3
        ent = ns * len(case.rc_of_strand)
        tiles = (ent * t3p + 255) // 256
        assert tiles > 1 and 4 * tiles > seam and 32 * ent > edge, (cid, tiles, ent)
        seam, edge = 4 * tiles, 32 * ent
        grown = fused.device_bytes() - plain.device_bytes() - base
        print(cid, "segments", ns, "conv4 tiles", tiles, "seam + edge bytes", grown)
        assert grown == (seam + edge) * 480 * 4, (cid, grown, seam, edge)


@pytest.mark.parametrize("precision", ["bf16x6", "fp32"])
@pytest.mark.parametrize("cid", ["L2204-0_200_204-both", "L2004-0_4-both"])
def test_other_arithmetics(setup, cid, precision):
    """pool4_phases in the other activation formats; and the f16x3 call right after it, over workspaces
    that then hold the other format's bits in the rows no window reads: no overflow fallback."""
    eng, sd = setup
    with eng.precision_override(precision):
        run_case(eng, sd, BY_ID[cid])
    run_case(eng, sd, BY_ID[cid], f64=False)


def test_strand_merge_knob_keeps_the_bits(setup):
    eng, sd = setup
    case = BY_ID["L2204-0_200_204-both"]
    a = run_case(eng, sd, case, f64=False)
    b = run_case(_knob_engine(EXPECTO_SEG_MERGE_STRANDS="0"), sd, case, f64=False)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
