"""Probe weights (oracle/probes.py) on the CPU: construction, coverage and sensitivity.

* Construction: the float64 forward of every level's probe network carries, hidden column by hidden
  column, exactly the chosen activations of the seeded network, and its pre-sigmoid values are
  a * act + b inside [-2, 2] (a, b from the float64 reference alone).
* Coverage: the conv6 selections hold the seam channels, the Karatsuba block edges and both sides of
  every FC1 slab seam; the tap sets show every conv5 / pool2 position and every conv3 / pool1 row
  that feeds the network, in pool groups of all four alignments.
* Sensitivity: with the float32 CPU forward standing in for a kernel, a relative 1e-3 on ONE conv6
  element or ONE FC1 column fails the probe comparison (tests/test_gpu_probe_weights.py's bar) and
  passes the dense seeded network under conftest.assert_close: the gap the probes close.
"""
import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import probes as P

SPECS = P.probe_specs()


@pytest.fixture(scope="module")
def ref():
    """The seeded network's stages on one window and its reverse complement, float64 and float32."""
    from expecto_amd.encode import codes_to_onehot
    x = codes_to_onehot(P.probe_codes()[:1], with_rc=True)
    sd = P.base_state_dict()
    return x, P.layer_activations(sd, x), P.layer_activations(sd, x, torch.float32)


@pytest.mark.parametrize("name", ["fc1-pos", "fc1-neg", "fc1-last", "6-sel0", "5-tap7", "4-tap7", "3-tap5", "2-tap6"])
def test_probe_network_carries_the_chosen_activations(ref, name):
    x, a64, a32 = ref
    p = P.probe(**SPECS[name]).set_scale(a64)
    got = P.layer_activations(p.sd, x)
    want = p.exposed(a64)
    assert torch.equal(got["fc1"], want)                     # copied by 0 / 1 weights: exact
    if p.level != "fc1":
        lvl = P.STAGE[p.level]
        assert torch.equal(got[lvl], a64[lvl])               # the layers up to the level are the seeded ones
        e = torch.from_numpy(p.entries)
        assert torch.equal(got["conv6"][:, e[:, 0], e[:, 1]], want)      # flatten order c * 106 + t
    pre = p.pre(a64)
    assert torch.equal(got["fc2_pre"], pre)
    assert float(pre.min()) >= -2.0 and float(pre.max()) <= 2.0 and float(pre.max()) > 1.999
    slope = torch.sigmoid(pre) * (1 - torch.sigmoid(pre))
    assert float(slope.min()) >= P.MIN_SLOPE
    assert float((p.visible(a64) > 0).double().mean()) > 0.3       # the outputs show activations, not sigmoid(b)
    # the float32 forward of the probe network is the float32 activations through the same copies
    got32 = P.layer_activations(p.sd, x, torch.float32)
    assert torch.equal(got32["fc1"], p.exposed(a32))
    assert float((got32["y"] - p.y(a32)).abs().max()) <= 1.2e-7


def test_fc1_probes_show_every_column(ref):
    _, a64, _ = ref
    pos, neg, last = (P.probe(**SPECS[n]) for n in ("fc1-pos", "fc1-neg", "fc1-last"))
    assert torch.equal(pos.visible(a64), a64["fc1"][:, :2002])
    assert torch.equal(last.visible(a64)[:, -1], a64["fc1"][:, 2002])
    shown = (pos.exposed(a64) > 0) | (neg.exposed(a64) > 0)          # one sign of every column
    assert bool(shown.all())


def test_conv6_selections_cover_seams_and_block_edges():
    sels = P.conv6_selections()
    have = set()
    for s in sels:
        assert s.shape == (P.N_HIDDEN, 2) and len({(int(c), int(t)) for c, t in s}) == P.N_HIDDEN
        have |= {(int(c), int(t)) for c, t in s}
    for c in (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 319, 320, 479, 480, 639):
        assert all((c, t) in have for t in range(106)), c
    for t in (0, 24, 25, 49, 50, 74, 75, 99, 100, 105):
        assert all((c, t) in have for c in range(640)), t
    for k_of in (lambda c, t: t * 640 + c, lambda c, t: c * 106 + t):      # kernel K order, reference order
        ks = {k_of(c, t) for c, t in have}
        for seam in range(8480, 67840, 8480):
            assert seam - 1 in ks and seam in ks, seam


def _groups(names, level):
    """{(channel, first row, last row)} of the stage's rows behind the outputs of these probes."""
    C, T = P.STAGE_SHAPE[level]
    first = {P.STAGE[level]: -torch.arange(T, dtype=torch.float64).expand(1, C, T)}
    last = {P.STAGE[level]: torch.arange(T, dtype=torch.float64).expand(1, C, T)}
    out = set()
    for n in names:
        p = P.probe(**SPECS[n])
        lo, hi = -p.exposed(first)[0], p.exposed(last)[0]
        out |= {(int(c), int(a), int(b)) for c, a, b in zip(p.entries[:, 0], lo, hi)}
    return out


def test_taps_show_every_position():
    g5 = _groups(["5-tap0", "5-tap7"], 5)
    assert all(a == b for _, a, b in g5)
    g4 = _groups(["4-tap0", "4-tap7"], 4)
    for c in (0, 255, 256, 639):
        assert {a for ch, a, _ in g5 if ch == c} == set(range(113)), c
    for c in (0, 255, 256, 479):
        assert {a for ch, a, _ in g4 if ch == c} == set(range(120)), c
    assert max(ch for ch, _, _ in g4) == 479
    for level, last_row, cmax in ((3, 486, 480), (2, 493, 320)):
        g = _groups([f"{level}-tap{t}" for t in range(8)], level)
        assert all(b - a == 3 for _, a, b in g)                         # pool groups of four
        assert max(ch for ch, _, _ in g) == cmax - 1
        for c in (0, 255, 256, cmax - 1):
            starts = {a for ch, a, _ in g if ch == c}
            rows = {r for a in starts for r in range(a, a + 4)}
            assert rows == set(range(last_row + 1)), (level, c)
            for r in range(64, 424):                                    # every alignment of the group holding r
                assert {r - a for a in starts if a <= r < a + 4} == {0, 1, 2, 3}, (level, c, r)


def _dense_tail(a32, conv6=None, fc1_pre=None):
    """The seeded network's float32 outputs from a (corrupted) conv6 or FC1 pre-activation on."""
    import torch.nn.functional as F
    from oracle.beluga_np import FC1_KEY, FC2_KEY
    sd = P.base_state_dict()
    with torch.no_grad():
        if fc1_pre is None:
            fc1_pre = F.linear(conv6.reshape(conv6.shape[0], -1), sd[FC1_KEY + ".weight"], sd[FC1_KEY + ".bias"])
        return torch.sigmoid(F.linear(F.relu(fc1_pre), sd[FC2_KEY + ".weight"], sd[FC2_KEY + ".bias"]))


@pytest.mark.parametrize("what", ["conv6", "fc1"])
def test_probes_catch_one_corrupted_activation_the_dense_network_hides(ref, what):
    _, a64, a32 = ref
    p = P.probe(**SPECS["6-sel0" if what == "conv6" else "fc1-pos"]).set_scale(a64)
    y64 = p.y(a64).numpy()
    limit, e_ref = P.bar(p.y(a32).numpy(), y64)
    assert np.abs(p.y(a32).numpy() - y64).max() <= limit                 # the stand-in itself passes
    # one element of typical size: the median of the positive shown values of window 0
    v = p.visible(a64)[0]
    j = int(torch.argsort(v)[int((v <= 0).sum()) + int((v > 0).sum()) // 2])
    bad = {k: t.clone() for k, t in a32.items()}
    if what == "conv6":
        c, t = (int(i) for i in p.entries[j + p.offset])
        bad["conv6"][0, c, t] *= 1 + 1e-3
        y_dense = _dense_tail(bad, conv6=bad["conv6"])
    else:
        bad["fc1_pre"][0, j] *= 1 + 1e-3
        bad["fc1"] = torch.relu(bad["fc1_pre"])
        y_dense = _dense_tail(bad, fc1_pre=bad["fc1_pre"])
    err = np.abs(p.y(bad).numpy() - y64)
    assert err.max() > limit, (err.max(), limit)
    assert np.unravel_index(err.argmax(), err.shape) == (0, j)          # and says where
    assert (err > limit).sum() == 1
    y_dense = y_dense.numpy()
    assert np.abs(y_dense - a32["y"].numpy()).max() > 0                  # the corruption reached the outputs
    assert_close(y_dense, a64["y"].numpy(), what="dense network, one corrupted activation")
