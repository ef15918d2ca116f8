"""FC stage of a segment chunk with the block-Karatsuba FC1: one grouped FC1 launch per slice that
also holds the alt windows' changed partials (out of place, after the ref partial rows), one
reduction over ref and alt windows.  Only the launch and the row a partial rides in change, so every
output equals, bit for bit (torch.equal), the in-place alt pass (EXPECTO_FC1K_ALT_INPLACE=1), one
chain per strand (EXPECTO_SEG_MERGE_STRANDS=0), the same chunk in several slices, and the per-window
forward of every window in its FC1 role.

Shapes: 200-bp sweeps of 200 shifts (both pool2 phases, 10 alt windows per strand and SNV whose
cones run through every block of their groups and their tails), rows="variant", seeded weights,
f16x3; max_batch 256 holds 2 or 3 SNVs' both strands (840 / 1260 FC rows) in one chunk and one slice
of 5 x 256."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import sweep_in_roles

pytestmark = pytest.mark.gpu

MAX_BATCH = 256
FULL = list(range(-20000, 20000, 200))
# the same sweep 52 bases on: the SNV's changed conv6 rows move 3 rows against the group starts
MOVED = [s + 52 for s in FULL]
# missing windows: groups of 1-3 windows, alt windows whose group lacks products
SPARSE = [s for j, s in enumerate(FULL) if j % 7 not in (2, 3) and j not in (97, 99, 102)]
HALF = list(range(-10000, 10000, 200))
_ENGINES = {}
_BASE = {}


def _engine(max_batch=MAX_BATCH, **env):
    """Seeded handles with the same weights, one per knob setting."""
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
    fa = Fasta.from_dict(g)
    snv = synthetic.snvs(g, 3, seed=9, margin=30_000)
    vs = VariantSet([s[0] for s in snv], np.array([s[1] for s in snv]), [s[2] for s in snv], [s[3] for s in snv])
    yield fa, DeviceGenome(fa), vs
    _ENGINES.clear()
    _BASE.clear()


def _predict(eng, setup, shifts, n_var, rows="variant"):
    from expecto_amd.pipeline import VariantPipeline
    fa, dg, vs = setup
    pipe = VariantPipeline(eng, fa, dg)
    y = pipe.predict(pipe.prepare(vs.slice(0, n_var), shifts, rows)).clone()
    torch.cuda.synchronize()
    return y


def _default(setup, name, shifts, n_var):
    """The default schedule's result of a sweep in one slice, computed once."""
    if name not in _BASE:
        _BASE[name] = _predict(_engine(), setup, shifts, n_var)
    return _BASE[name]


def _same(got, want, what):
    assert got.shape == want.shape
    assert torch.equal(got, want), f"{what}: max|diff| {float((got - want).abs().max())}"


@pytest.mark.parametrize("name,shifts", [("full", FULL), ("moved", MOVED), ("sparse", SPARSE)])
def test_alt_rows_in_the_ref_launch(setup, name, shifts):
    """2 SNVs x both strands: the default against the in-place alt pass and one chain per strand."""
    got = _default(setup, name, shifts, 2)
    assert got.shape[:3] == (2, 2, 2) and bool((got[:, 0] != got[:, 1]).any())   # alt rows differ from ref rows
    _same(got, _predict(_engine(EXPECTO_FC1K_ALT_INPLACE="1"), setup, shifts, 2), "in place")
    _same(got, _predict(_engine(EXPECTO_SEG_MERGE_STRANDS="0"), setup, shifts, 2), "per strand")


@pytest.mark.parametrize("inplace", ["0", "1"])
def test_slices(setup, inplace):
    """3 SNVs x 100 shifts on a handle of max_batch 20 (its workspace holds one segment of 21,800
    bases) with the slice capped at it: a chunk is one (strand, SNV) entry of 100 windows in 6 or more
    slices, and out of place its 4 alt groups (16 windows + 10 alt windows = 26 FC rows) do not fit
    the first (tests/test_fc_stage_plan.py pins that cut on the host).  Equal to the one-slice run."""
    want = _default(setup, "half3", HALF, 3)
    got = _predict(_engine(20, EXPECTO_FC1K_SLICE="20", EXPECTO_FC1K_ALT_INPLACE=inplace), setup, HALF, 3)
    _same(got, want, "sliced")


def test_windows_in_their_roles(setup):
    """One SNV: every window of the sweep, ref and alt, equals its per-window forward in its role."""
    from expecto_amd.pipeline import VariantPipeline
    fa, dg, vs = setup
    one = (fa, dg, vs.slice(1, 2))
    eng = _engine()
    got = _predict(eng, one, FULL, 1, rows="shift")
    pipe = VariantPipeline(eng, fa, dg, use_segments=False, use_pairs=False)
    want = sweep_in_roles(eng, lambda: pipe.predict(one[2], FULL), FULL)
    for s in range(2):
        _same(got[s], want[s], f"strand {s}")
