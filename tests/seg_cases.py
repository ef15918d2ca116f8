"""Shared logic of tests/test_gpu_segment_geometry.py: the segment path's geometry cases (segment
length, window offsets, strand mode, the pool2 phase set and T4 % 4 they must reach), their inputs,
and the comparison of a segment call with per-window forwards.

A case's windows are compared bit for bit with forward_codes of each window's own 2000 codes, the
window taken in the FC1 role the segment path gives it (pipeline.fc1_role; role 4, the direct FC1,
when more than a third of a pairs call's windows hold the SNV), and its first and last window of
segment 0 with a float64 forward (oracle/beluga_np.py) at the project's parity bar."""
import os

import numpy as np
import torch

from conftest import assert_close, run_in_roles

FWD, RC, BOTH = 0, 1, 2          # expecto_amd._lib.STRAND_*
MODE_NAME = {FWD: "fwd", RC: "rc", BOTH: "both"}
L_MAX = 2220
N_SEG = 3


class Case:
    """L, the window offsets of every segment, the strand mode; the phase set and T4 % 4 the case is
    there for (hand arithmetic, asserted against seg_plan's rule), and the pool2 path: 'fused' (conv4's
    epilogue, phases exactly {0, 2}) or 'pass' (the separate pool pass)."""

    def __init__(self, L, offs, mode, phases, t4_mod, pool="pass"):
        self.L, self.offs, self.mode, self.phases, self.t4_mod, self.pool = L, tuple(offs), mode, set(phases), t4_mod, pool

    @property
    def id(self):
        return f"L{self.L}-{'_'.join(map(str, self.offs))}-{MODE_NAME[self.mode]}"

    @property
    def rc_of_strand(self):
        """rc flag of every computed strand, in output order."""
        return {FWD: [False], RC: [True], BOTH: [False, True]}[self.mode]


def phase_set(L, offs, mode):
    """seg_plan's rule (expecto_amd/csrc/seg_plan.h), as tests/test_seg_plan.py n_phases restates it."""
    ph = set()
    for o in offs:
        if mode != RC:
            ph.add((o >> 2) & 3)
        if mode != FWD:
            ph.add(((L - 2000 - o) >> 2) & 3)
    return ph


def t4_of(L):
    return (L - 14) // 4 - 14


# Offset L - 2000 is in phase 1 for L = 2212 (212 = 4 x 53) and in phase 3 for L = 2220 (220 = 4 x 55) on
# the fwd strand, so the cases that must reach exactly {0, 2} on a strand cannot hold it: they end at
# L - 2004 (208, phase 0; 216, phase 2), and the last base of their segments lies in no window.  Every
# other case holds offset 0 and offset L - 2000.
CASES = [
    Case(2000, [0], FWD, {0}, 2),
    Case(2000, [0], RC, {0}, 2),
    Case(2000, [0], BOTH, {0}, 2),
    Case(2016, [0, 16], BOTH, {0}, 2),
    Case(2008, [0, 8], BOTH, {0, 2}, 0, "fused"),
    Case(2004, [0, 4], BOTH, {0, 1}, 3),
    Case(2012, [0, 12], BOTH, {0, 3}, 1),
    Case(2204, [0, 200, 204], FWD, {0, 2, 3}, 1),
    Case(2204, [0, 200, 204], RC, {3, 1, 0}, 1),
    Case(2204, [0, 200, 204], BOTH, {0, 1, 2, 3}, 1),
    Case(2204, [0, 204], RC, {3, 0}, 1),
    Case(2212, [0, 8, 200, 208], FWD, {0, 2}, 3, "fused"),
    Case(2212, [0, 8, 200, 208], BOTH, {0, 1, 2, 3}, 3),
    Case(2220, [0, 200, 216], FWD, {0, 2}, 1, "fused"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def check_geometry(case):
    """The case reaches what it is listed for."""
    assert case.L >= 2000 and case.L % 4 == 0 and all(o % 4 == 0 and 0 <= o <= case.L - 2000 for o in case.offs)
    assert phase_set(case.L, case.offs, case.mode) == case.phases, case.id
    assert t4_of(case.L) % 4 == case.t4_mod, case.id
    if case.mode == BOTH and len(case.phases) == 4 and case.L % 16 in (4, 12) and len(case.offs) == 4:
        f, r = phase_set(case.L, case.offs, FWD), phase_set(case.L, case.offs, RC)
        assert len(f) == len(r) == 2 and not f & r, case.id      # two phases per strand, disjoint
    assert (case.pool == "fused") == (case.phases == {0, 2})


_BASE = np.random.default_rng(20260).integers(0, 5, (8, L_MAX)).astype(np.uint8)   # codes 0..4: N included


def segment_codes(L, ns=N_SEG):
    """ns segments of L codes: prefixes of one random table, so the window at offset 0 is the same
    window in every case."""
    return np.ascontiguousarray(_BASE[:ns, :L])


class Windows:
    """Window tables of a call: offs[s] for segment s, sorted by segment; output rows a fixed
    permutation of the windows (not the identity)."""

    def __init__(self, offs_per_seg):
        self.seg = np.array([s for s, offs in enumerate(offs_per_seg) for _ in offs], np.int32)
        self.off = np.array([o for offs in offs_per_seg for o in offs], np.int32)
        n = self.n = self.seg.size
        self.row = ((np.arange(n) * 5 + 3) % n if n % 5 else n - 1 - np.arange(n)).astype(np.int32)
        assert sorted(self.row) == list(range(n))

    def cut(self, codes):
        return np.stack([codes[s, o:o + 2000] for s, o in zip(self.seg, self.off)])


def want_rows(eng, case, codes, win, direct):
    """[strands, n_win, 2002]: forward_codes of every window in its FC1 role."""
    from expecto_amd.pipeline import fc1_role
    rcs = case.rc_of_strand
    wins = torch.from_numpy(win.cut(codes)).cuda()
    by_role = run_in_roles(eng, lambda: eng.forward_codes(wins, case.mode).view(len(rcs), win.n, 2002))
    out = torch.empty_like(by_role[4])
    for si, rc in enumerate(rcs):
        for w in range(win.n):
            out[si, w] = by_role[4 if direct else fc1_role(int(win.off[w]), case.L, rc)][si, w]
    return out


def same_rows(got, want, case, win, what):
    """got [strands * n_win, 2002] in the call's row order == want [strands, n_win, 2002]."""
    ns = len(case.rc_of_strand)
    g = got.view(ns, win.n, 2002)[:, torch.from_numpy(win.row.astype(np.int64)).cuda()]
    if torch.equal(g, want):
        return
    d = (g - want).abs().amax(-1)
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).cpu().numpy()
    bad = [(("rc" if case.rc_of_strand[s] else "fwd"), int(win.seg[w]), int(win.off[w]), float(d[s, w]))
           for s in range(ns) for w in range(win.n) if d[s, w] != 0 or not torch.equal(g[s, w], want[s, w])]
    raise AssertionError(f"{case.id} {what}: (strand, segment, offset, max|diff|; inf: NaN, a row not written) {bad}")


_Y64 = {}


def float64_rows(sd, window):
    """[2, 2002] float64 forward of a window's codes, fwd and rc (cached by the window)."""
    from expecto_amd.encode import codes_to_onehot
    from oracle.beluga_np import forward_torch_cpu
    key = window.tobytes()
    if key not in _Y64:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        x = torch.from_numpy(codes_to_onehot(window[None], with_rc=True).astype(np.float64)).unsqueeze(2)
        if "sd" not in _Y64:
            _Y64["sd"] = {k: v.double() for k, v in sd.items()}
        _Y64[key] = forward_torch_cpu(_Y64["sd"], x).numpy()
    return _Y64[key]


def check_float64(got, sd, case, codes, win, what):
    """Segment 0's first and last window on every computed strand against the float64 forward."""
    mine = [w for w in range(win.n) if win.seg[w] == 0]
    for w in (mine[0], mine[-1]):
        y64 = float64_rows(sd, codes[0, win.off[w]:win.off[w] + 2000])
        for si, rc in enumerate(case.rc_of_strand):
            row = got.view(len(case.rc_of_strand), win.n, 2002)[si, int(win.row[w])].cpu().numpy()
            assert_close(row, y64[int(rc)], what=f"{case.id} {what} offset {win.off[w]} {'rc' if rc else 'fwd'} vs float64")


def snv_positions(L):
    return sorted({min(max(q, 0), L - 1) for q in (0, 7, 8, L - 2000 - 1, L - 2000, 1999, 2000, L - 1)})


def pair_calls(case, ns=N_SEG):
    """The pairs calls of a case: per call (q, kind, offsets) per segment.  The SNV positions, ns per
    call (the last call filled up from the start of the list); kind 'n': alt code N, 'same': the
    reference base, 'snv': another base -- one segment of each kind in a call, rotating.  The segment
    whose SNV is the last base keeps only the offsets <= L - 2004 when L > 2004, so no window holds
    its SNV (its kind is 'snv': an alt run spliced where none belongs would show)."""
    qs = snv_positions(case.L)
    calls = []
    for k in range(0, len(qs), ns):
        part = (qs[k:k + ns] + qs)[:ns]
        call = []
        for s, q in enumerate(part):
            kind = ("n", "same", "snv")[(s + k // ns) % 3] if ns >= 3 else "snv"
            offs = list(case.offs)
            if q == case.L - 1 and case.L > 2004:
                offs, kind = [o for o in offs if o <= case.L - 2004], "snv"
            call.append((q, kind, offs))
        calls.append(call)
    return calls


def alt_codes(codes, call, rng):
    ref = np.array([codes[s, q] for s, (q, _, _) in enumerate(call)])
    alt = np.array([4 if kind == "n" else b if kind == "same" else (b + 1 + rng.integers(0, 3)) % 4
                    for b, (_, kind, _) in zip(ref, call)], np.uint8)
    spliced = codes.copy()
    spliced[np.arange(len(call)), [q for q, _, _ in call]] = alt
    return alt, spliced


def check_pair_coverage(case, calls):
    """The pairs calls place an SNV in every window, in exactly one window and (L >= 2204) in none."""
    held = [sum(o <= q < o + 2000 for o in offs) for call in calls for q, _, offs in call]
    n_w = [len(offs) for call in calls for _, _, offs in call]
    kinds = {kind for call in calls for _, kind, _ in call}
    assert any(h == n and n == len(case.offs) for h, n in zip(held, n_w)), case.id
    assert any(h == 1 for h in held), case.id
    assert case.L < 2204 or any(h == 0 for h in held), case.id
    assert kinds == {"n", "same", "snv"}, case.id


def run_case(eng, sd, case, ns=N_SEG, f64=True):
    """forward_segments once and forward_segment_pairs (once per ns SNV positions) on the case; every
    window, ref and alt, on every computed strand, against forward_codes of its own codes; the
    fallback count unchanged.  Returns the outputs (for a bit comparison with another handle)."""
    check_geometry(case)
    calls = pair_calls(case, ns)
    check_pair_coverage(case, calls)
    n0 = eng.f16_state()[0]
    nst = len(case.rc_of_strand)
    codes = segment_codes(case.L, ns)
    codes_d = torch.from_numpy(codes).cuda()
    outs = []
    win = Windows([case.offs] * ns)
    want = want_rows(eng, case, codes, win, direct=False)
    y = torch.full((nst * win.n, 2002), float("nan"), device="cuda")
    eng.forward_segments(codes_d, case.L, win.seg, win.off, win.row, case.mode, out=y)
    same_rows(y, want, case, win, "forward_segments")
    if f64:
        check_float64(y, sd, case, codes, win, f"forward_segments ({eng.precision})")
    outs.append(y)
    rng = np.random.default_rng(case.L)
    for k, call in enumerate(calls):
        win = Windows([offs for _, _, offs in call])
        q = np.array([c[0] for c in call], np.int32)
        alt, spliced = alt_codes(codes, call, rng)
        n_alt = int(((win.off <= q[win.seg]) & (q[win.seg] < win.off + 2000)).sum())
        direct = 3 * n_alt > win.n
        y_ref = torch.full((nst * win.n, 2002), float("nan"), device="cuda")
        y_alt = torch.full((nst * win.n, 2002), float("nan"), device="cuda")
        eng.forward_segment_pairs(codes_d, case.L, q, torch.from_numpy(alt).cuda(), win.seg, win.off, win.row, y_ref,
                                  y_alt, win.n, case.mode)
        what = f"pairs call {k} (q {q.tolist()}, alt {alt.tolist()}, {'direct' if direct else 'Karatsuba'} FC1)"
        same_rows(y_ref, want_rows(eng, case, codes, win, direct), case, win, what + " ref")
        same_rows(y_alt, want_rows(eng, case, spliced, win, direct), case, win, what + " alt")
        if f64 and k == 0:
            check_float64(y_ref, sd, case, codes, win, f"pairs ref ({eng.precision})")
        outs += [y_ref, y_alt]
    torch.cuda.synchronize()
    assert eng.f16_state()[0] == n0, f"{case.id}: an f16x3 overflow fallback ran"
    return outs
