"""Probe weights: Beluga networks whose 2002 outputs each show ONE activation of a chosen layer
-- TEST INFRASTRUCTURE (oracle) ONLY, CPU only.

The dense seeded network averages 67,840 conv6 values into every FC1 pre-activation and 2,003
hidden values into every output, so a fault in one activation reaches the outputs diluted to about
1e-5, inside the parity bar.  A probe network keeps the seeded weights (oracle/weights.py, seed 0,
gain sqrt 6) up to the layer under test and replaces what follows by layers that only move values:

* ``passthrough_conv``  one 1.0 per output channel: out[c, t] = in[c, t + tap];
* ``fc1_selector``      one-hot rows: hidden j = conv6[c_j, t_j] (flat index c * 106 + t, Beluga.py:42);
* ``fc2_identity``      output j = sigmoid(a * hidden[j + offset] + b).

conv1 and conv2 always keep the seeded weights, so every probe engine shares the seeded engine's
k-mer tables.  ``Probe.exposed`` says, by index arithmetic alone (copies and pool maxima, exact in
any number format), which activation of the seeded network each hidden column carries;
``layer_activations`` is the plain torch-CPU forward (graph of oracle/beluga_np.forward_torch_cpu)
that returns every stage.
"""
from __future__ import annotations

import functools

import numpy as np

from .beluga_np import CONV_KEYS, FC1_KEY, FC2_KEY

CONV_SHAPES = ((320, 4), (320, 320), (480, 320), (480, 480), (640, 480), (640, 640))   # (cout, cin) of conv1..conv6
N_HIDDEN = 2003
N_OUT = 2002
T6 = 106                      # conv6 positions; FC1 reads 640 * 106 = 67840 values
FC1_IN = 640 * T6
STAGE = {2: "pool1", 3: "conv3", 4: "pool2", 5: "conv5", 6: "conv6"}
STAGE_SHAPE = {2: (320, 496), 3: (480, 489), 4: (480, 120), 5: (640, 113), 6: (640, 106)}
LEVELS = (2, 3, 4, 5, 6, "fc1")
B_OFFSET = -2.0               # pre-sigmoid values a * act + b with a = 4 / amax lie in [-2, 2]
MIN_SLOPE = 0.104             # sigmoid'(2) = 0.10499: the least slope on [-2, 2]

# channels on both sides of every power-of-two seam from 16 to 512, of the 320 / 480 layer widths, and the last
SEAM_CHANNELS = (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 319, 320, 479, 480, 511, 512, 639)
# first / last rows of the 25-row Karatsuba blocks of FC1 (include/expecto_hip.h) and of the 6-row tail
BLOCK_EDGES = (0, 24, 25, 49, 50, 74, 75, 99, 100, 105)
FC1_SLAB = 8480               # FC1 split-K slab (8 slabs of 67840)


def layer_activations(sd: dict, x, dtype=None) -> dict:
    """Every stage of Beluga.forward (Beluga.py:18-51), each after its ReLU, as torch tensors:
    conv1 [n,320,1993], pool1 (conv2 + pool) [n,320,496], conv3 [n,480,489], pool2 (conv4 + pool)
    [n,480,120], conv5 [n,640,113], conv6 [n,640,106], fc1_pre / fc1 [n,2003], fc2_pre [n,2002] and
    y = sigmoid(fc2_pre).  x: [n,4,2000] or [n,4,1,2000]; dtype: torch.float64 (default) or float32."""
    import torch
    import torch.nn.functional as F

    dtype = dtype or torch.float64
    g = lambda k: sd[k].to(dtype)
    x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(dtype)
    if x.dim() == 3:
        x = x.unsqueeze(2)
    names = ("conv1", "pool1", "conv3", "pool2", "conv5", "conv6")
    out = {}
    with torch.no_grad():
        h = x
        for i, key in enumerate(CONV_KEYS):
            h = F.relu(F.conv2d(h, g(key + ".weight"), g(key + ".bias")))
            if i in (1, 3):
                h = F.max_pool2d(h, (1, 4), (1, 4))
            out[names[i]] = h[:, :, 0, :]
        flat = h.reshape(h.shape[0], -1)
        out["fc1_pre"] = F.linear(flat, g(FC1_KEY + ".weight"), g(FC1_KEY + ".bias"))
        out["fc1"] = F.relu(out["fc1_pre"])
        out["fc2_pre"] = F.linear(out["fc1"], g(FC2_KEY + ".weight"), g(FC2_KEY + ".bias"))
        out["y"] = torch.sigmoid(out["fc2_pre"])
    return out


@functools.lru_cache(maxsize=1)
def base_state_dict() -> dict:
    """The golden vectors' weights (seed 0, gain sqrt 6); shared by every probe, never modified."""
    from .weights import seeded_state_dict
    return seeded_state_dict(0)


def passthrough_conv(cout: int, cin: int, tap: int):
    """(weight [cout,cin,1,8], bias): W[c, c, 0, tap] = 1 for c < min(cin, cout), so out[c, t] = in[c, t + tap]."""
    import torch
    assert 0 <= tap < 8
    w = torch.zeros((cout, cin, 1, 8), dtype=torch.float32)
    c = torch.arange(min(cin, cout))
    w[c, c, 0, tap] = 1.0
    return w, torch.zeros(cout, dtype=torch.float32)


def fc1_selector(entries, scale: float = 1.0):
    """(weight [2003,67840], bias): row j is one-hot at flat index c * 106 + t of the j-th (c, t)."""
    import torch
    e = np.asarray(entries, np.int64)
    assert e.shape == (N_HIDDEN, 2) and (e >= 0).all() and (e[:, 0] < 640).all() and (e[:, 1] < T6).all()
    w = torch.zeros((N_HIDDEN, FC1_IN), dtype=torch.float32)
    w[torch.arange(N_HIDDEN), torch.from_numpy(e[:, 0] * T6 + e[:, 1])] = scale
    return w, torch.zeros(N_HIDDEN, dtype=torch.float32)


def fc2_identity(a: float, b: float, offset: int = 0):
    """(weight [2002,2003], bias): W[j, j + offset] = a, bias b; offset 1 shows hidden column 2002."""
    import torch
    assert offset in (0, 1)
    w = torch.zeros((N_OUT, N_HIDDEN), dtype=torch.float32)
    j = torch.arange(N_OUT)
    w[j, j + offset] = a
    return w, torch.full((N_OUT,), b, dtype=torch.float32)


def slab_seam_entries():
    """conv6 entries (c, t) on both sides of every FC1 split-K slab seam (multiples of 8480), in the
    kernel's K order t * 640 + c (beluga.hip repack_fc1) and in the reference's c * 106 + t."""
    out = []
    for s in range(1, FC1_IN // FC1_SLAB):
        for k in (s * FC1_SLAB - 1, s * FC1_SLAB):
            out.append((k % 640, k // 640))
            out.append((k // T6, k % T6))
    return sorted(set(out))


def _fill(must, cmax: int, seed: int):
    """`must` (unique entries) + random further entries with c < cmax, 2003 in all, shuffled so that
    no hidden column's index is tied to its entry's channel or position."""
    rng = np.random.default_rng(seed)
    must = list(dict.fromkeys((int(c), int(t)) for c, t in must))
    assert len(must) <= N_HIDDEN and all(c < cmax for c, _ in must)
    have = set(must)
    while len(must) < N_HIDDEN:
        e = (int(rng.integers(0, cmax)), int(rng.integers(0, T6)))
        if e not in have:
            have.add(e)
            must.append(e)
    e = np.array(must, np.int64)
    return e[rng.permutation(N_HIDDEN)]


def conv6_selections():
    """Five selections of 2003 conv6 entries that together hold every position of SEAM_CHANNELS,
    every channel at BLOCK_EDGES and both sides of every FC1 slab seam."""
    sels = [_fill([(c, t) for c in SEAM_CHANNELS for t in range(T6)] + slab_seam_entries(), 640, 60)]
    edge = [(c, t) for t in BLOCK_EDGES for c in range(640)]
    for i in range(4):
        sels.append(_fill(edge[i * 1600:(i + 1) * 1600], 640, 61 + i))
    return sels


def channel_selection(cmax: int, seed: int = 0):
    """Every position of the SEAM_CHANNELS below cmax, further channels up to 18 in all, and random
    entries of the first cmax channels: what the probes of the layers before conv6 select."""
    ch = [c for c in SEAM_CHANNELS if c < cmax]
    extra = [c for c in (cmax - 1, 159, 160, 95, 96, 191, 192, 383, 384, 447, 448) if c < cmax and c not in ch]
    ch += extra[:18 - len(ch)]
    return _fill([(c, t) for c in ch for t in range(T6)], cmax, 50 + seed)


class Probe:
    """A probe network: `sd` (fp32 state dict), and `exposed(acts)`, the hidden vector [n, 2003] it
    must carry given the seeded network's `layer_activations`."""

    def __init__(self, level, taps=None, entries=None, negate=False, offset=0, gain_log2=0):
        assert level in LEVELS
        self.level, self.negate, self.offset, self.gain_log2 = level, bool(negate), int(offset), int(gain_log2)
        self.taps = dict(taps or {})
        self.a = None
        self.b = B_OFFSET
        base = base_state_dict()
        sd = dict(base)
        if level == "fc1":
            assert not self.taps and entries is None
            self.entries = None
            if negate:
                sd[FC1_KEY + ".weight"] = -base[FC1_KEY + ".weight"]
                sd[FC1_KEY + ".bias"] = -base[FC1_KEY + ".bias"]
        else:
            assert not negate and sorted(self.taps) == list(range(level + 1, 7))
            for l in range(level + 1, 7):
                w, bias = passthrough_conv(*CONV_SHAPES[l - 1], self.taps[l])
                sd[CONV_KEYS[l - 1] + ".weight"], sd[CONV_KEYS[l - 1] + ".bias"] = w, bias
            self.entries = np.asarray(entries, np.int64)
            assert (self.entries[:, 0] < STAGE_SHAPE[level][0]).all()
            # 2^gain_log2 on the selector and 2^-gain_log2 on a: the same function, other fp16 ranges
            sd[FC1_KEY + ".weight"], sd[FC1_KEY + ".bias"] = fc1_selector(self.entries, 2.0 ** self.gain_log2)
        del sd[FC2_KEY + ".weight"], sd[FC2_KEY + ".bias"]          # set_scale decides them
        self._sd = sd

    def conv6_view(self, acts):
        """What the pass-through layers leave at conv6's output [n, 640, 106]: copies (and pool
        maxima) of acts[STAGE[level]]."""
        import torch
        A = acts[STAGE[self.level]]
        for l in range(self.level + 1, 7):
            cout, cin = CONV_SHAPES[l - 1]
            tap, T = self.taps[l], A.shape[2] - 7
            B = torch.zeros((A.shape[0], cout, T), dtype=A.dtype)
            m = min(cin, cout)
            B[:, :m] = A[:, :m, tap:tap + T]
            if l in (2, 4):
                B = B[:, :, :T // 4 * 4].reshape(B.shape[0], cout, T // 4, 4).amax(dim=3)
            A = B
        return A

    def exposed(self, acts):
        """Hidden values [n, 2003] in acts' dtype (without the selector's power-of-two gain)."""
        import torch
        if self.level == "fc1":
            return torch.relu(-acts["fc1_pre"]) if self.negate else acts["fc1"]
        e = torch.from_numpy(self.entries)
        return self.conv6_view(acts)[:, e[:, 0], e[:, 1]]

    def visible(self, acts):
        """The hidden columns the 2002 outputs show, [n, 2002]."""
        return self.exposed(acts)[:, self.offset:self.offset + N_OUT]

    def set_scale(self, acts64):
        """a = 4 / amax from the float64 reference alone (amax: the largest shown activation), rounded
        down to fp32 so that the FC2 weight holds it exactly and a * amax <= 4."""
        amax = float(self.visible(acts64).max())
        assert amax > 0
        a = np.float32(4.0 / amax)
        while float(a) * amax > 4.0:
            a = np.nextafter(a, np.float32(0))
        self.a = float(a)
        return self

    @property
    def sd(self) -> dict:
        assert self.a is not None, "set_scale first"
        sd = dict(self._sd)
        sd[FC2_KEY + ".weight"], sd[FC2_KEY + ".bias"] = fc2_identity(self.a * 2.0 ** -self.gain_log2, self.b,
                                                                    self.offset)
        return sd

    def pre(self, acts):
        """Pre-sigmoid values a * act + b [n, 2002] in acts' dtype (the selector's 2^gain_log2 and
        FC2's a * 2^-gain_log2 are powers of two apart from a: the product rounds once either way)."""
        return self.visible(acts) * self.a + self.b

    def y(self, acts):
        import torch
        return torch.sigmoid(self.pre(acts))


def probe(level, taps=None, entries=None, negate=False, offset=0, gain_log2=0) -> Probe:
    """Layers 3..level keep the seeded weights, conv layers after `level` are pass-throughs with
    `taps` {layer: tap}, FC1 selects `entries` (the seeded FC1, negated if `negate`, for level
    "fc1") and FC2 is the scaled identity (call set_scale with the float64 activations)."""
    return Probe(level, taps, entries, negate, offset, gain_log2)


def probe_specs():
    """{name: keyword arguments of probe()} of every probe network the tests run, by level.

    fc1: the seeded network, negated (the columns below the ReLU), and offset 1 (column 2002).
    6:   conv6_selections().
    5:   conv6 copies conv5 at tap 0 (positions 0..105) and tap 7 (7..112).
    4:   conv5, conv6 taps (0, 0) and (7, 7): pooled positions 0..105 and 14..119, channels < 480.
    3:   conv4 + pool2 copy conv3: an output is the maximum of 4 consecutive conv3 rows from
         4 j + tap4; tap4 0..3 with (0, 0) and 4..7 with (7, 7) put every conv3 row 0..486 (what
         feeds the real network) in groups of all four alignments.
    2:   the same with conv3 as a copy at tap 0 (tap 7 for the far half): pool1 rows 0..493.
    """
    specs = {"fc1-pos": dict(level="fc1"), "fc1-neg": dict(level="fc1", negate=True),
             "fc1-last": dict(level="fc1", offset=1)}
    for i, sel in enumerate(conv6_selections()):
        specs[f"6-sel{i}"] = dict(level=6, taps={}, entries=sel)
    for tap in (0, 7):
        specs[f"5-tap{tap}"] = dict(level=5, taps={6: tap}, entries=channel_selection(640, tap))
        specs[f"4-tap{tap}"] = dict(level=4, taps={5: tap, 6: tap}, entries=channel_selection(480, tap))
    for t4 in range(8):
        far = 7 if t4 >= 4 else 0
        specs[f"3-tap{t4}"] = dict(level=3, taps={4: t4, 5: far, 6: far}, entries=channel_selection(480, t4))
        specs[f"2-tap{t4}"] = dict(level=2, taps={3: far, 4: t4, 5: far, 6: far}, entries=channel_selection(320, t4))
    return specs


def level_of(name: str):
    return "fc1" if name.startswith("fc1") else int(name[0])


def bar(y_ref32, y64, k: float = 3.0):
    """The project's accuracy rule (tests/test_gpu_forward.py::test_accuracy_vs_float64), element-wise
    on a probe's outputs: max|y - y64| <= k * e_ref + 1e-6 with e_ref the float32 CPU forward's error."""
    e_ref = float(np.abs(np.asarray(y_ref32, np.float64) - np.asarray(y64, np.float64)).max())
    return k * e_ref + 1e-6, e_ref


N_WIDE = 29     # windows of the test inputs: both strands are 58 rows, the smallest batch whose conv3..conv6
                # launches all leave the narrow tiles (tests/test_gpu_probe_weights.py)


def probe_codes(seed: int = 0, n: int = N_WIDE) -> np.ndarray:
    """Base codes uint8 [n, 2000] from rng.integers(0, 5): N columns (code 4) nearly everywhere, so
    the k-mer gather takes its 4-row path; window 3 has no N and takes the 2-row path."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 5, (n, 2000)).astype(np.uint8)
    if n > 3:
        codes[3] = rng.integers(0, 4, 2000).astype(np.uint8)
    return codes
