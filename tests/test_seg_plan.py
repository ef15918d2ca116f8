"""The segment path's host planner (expecto_amd/csrc/seg_plan.h), without a GPU: the header is built
with the host compiler alone into tests/seg_plan_driver.cpp, which prints the plan of every case it
reads.  Properties of every plan over a small grid, the figures the project's record pins (chunk
lists and FC1 modes of test_gpu_strand_merge.py, the headline's one chunk) and every refusal's text.
Nothing of the planner is restated here beyond the properties."""
import itertools
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, RC, BOTH = 0, 1, 2
FK_CAP = 24576   # the handle's default slice (EXPECTO_FC1K_SLICE)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seg_plan") / "seg_plan_driver")
    cxx = [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", os.path.join(REPO, "tests", "seg_plan_driver.cpp"), "-o", exe],
                   check=True)
    return exe


def _caps(max_batch):
    """Elements of P and Q that hold segment rows (beluga.hip p_floats / q_floats less their pad)."""
    return max_batch * 1996 * 320, max_batch * 496 * 320


def case(n_seg, L, mode, win_seg, win_off, max_batch, var_pos=None, win_row=None, merge=1, chunk_windows=0, fk=1,
         fk_cap=FK_CAP, caps=None):
    p_cap, q_cap = caps or _caps(max_batch)
    return dict(n_seg=n_seg, L=L, mode=mode, win_seg=list(win_seg), win_off=list(win_off), max_batch=max_batch,
                var_pos=var_pos, win_row=win_row, merge=merge, chunk_windows=chunk_windows, fk=fk, fk_cap=fk_cap,
                p_cap=p_cap, q_cap=q_cap)


def plans(driver, cases):
    """The driver's output for the cases: per case {field: [ints]}, 'chunk': [{fk_ref, fk_alt, gres,
    slices}], or {'error': message}."""
    text = []
    for c in cases:
        n = len(c["win_seg"])
        head = [c["n_seg"], c["L"], c["mode"], n, int(c["var_pos"] is not None), int(c["win_row"] is not None),
                c["max_batch"], c["p_cap"], c["q_cap"], c["merge"], c["chunk_windows"], c["fk"], c["fk_cap"],
                2 * n if c["var_pos"] is not None else n]
        text.append(" ".join(map(str, head + c["win_seg"] + c["win_off"] + (c["win_row"] or []) + (c["var_pos"] or []))))
    out = subprocess.run([driver], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout
    res, cur = [], None
    for ln in out.splitlines():
        name, _, rest = ln.partition(" ")
        if name == "case":
            cur = {"chunk": []}
        elif name == "end":
            res.append(cur)
        elif name in ("error", "slice_error"):
            cur[name] = rest
        else:
            v = [int(x) for x in rest.split()]
            if name == "fk_ref":
                cur["chunk"].append({})
            if name in ("fk_ref", "fk_alt", "gres", "slices"):
                cur["chunk"][-1][name] = v
            else:
                cur[name] = v
    assert len(res) == len(cases)
    return res


def sweep(n_seg, n_per, step, uneven=False):
    """n_per windows at `step` bp per segment (uneven: odd segments lack the first)."""
    win_seg, win_off = [], []
    for s in range(n_seg):
        for k in range(1 if uneven and s % 2 and n_per > 1 else 0, n_per):
            win_seg.append(s)
            win_off.append(k * step)
    return win_seg, win_off, 2000 + step * (n_per - 1)


def min_max_batch(L, n_ph):
    """The seg_cap arithmetic as tests/test_gpu_strand_merge.py::_min_max_batch restates it, less its
    n_ph floor: the smallest max_batch whose workspace holds one segment of L bases."""
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
    return max(-(-p // (1996 * 320)), -(-q // (496 * 320)))


def n_phases(c):
    ph = set()
    for o in c["win_off"]:
        if c["mode"] != RC:
            ph.add((o >> 2) & 3)
        if c["mode"] != FWD:
            ph.add(((c["L"] - 2000 - o) >> 2) & 3)
    return len(ph)


def check_plan(c, p):
    assert "error" not in p, (c, p)
    n_seg, n_win, L = c["n_seg"], len(c["win_seg"]), c["L"]
    strands = 2 if c["mode"] == BOTH else 1
    n_ent, n_vw = p["n_ent"][0], p["n_vw"][0]
    assert (n_ent, n_vw) == (strands * n_seg, strands * n_win)
    assert p["n_ph"][0] == n_phases(c)
    vfirst, pairs = p["vfirst"], c["var_pos"] is not None
    rc_win = p["ss"][3]
    assert rc_win == {FWD: n_vw, RC: 0, BOTH: n_win}[c["mode"]]
    is_alt = lambda v: bool(p["is_alt"][v % n_win])
    ent_of = lambda v: (v // n_win) * n_seg + c["win_seg"][v % n_win]
    # chunks: a partition of the entries in order, within the caps
    ch = list(zip(p["chunks"][::2], p["chunks"][1::2]))
    assert ch[0][0] == 0 and ch[-1][1] == n_ent and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
    blk = p["blk_per_seg"][0]
    assert blk == (max(p["n_ph"][0], 1) if pairs else 0)
    for e0, e1 in ch:
        assert 1 <= e1 - e0 <= p["seg_cap"][0]
        assert not blk or e1 - e0 <= c["max_batch"] // blk
        assert c["chunk_windows"] <= 0 or e1 - e0 == 1 or vfirst[e1] - vfirst[e0] <= c["chunk_windows"]
        assert c["merge"] or not e0 < n_seg < e1
    fkm = bool(p["fkm"][0])
    assert fkm == bool(c["fk"] and not (pairs and 3 * len(p["alt_w"]) > n_vw))
    assert sorted(p["alt_w"] + p["copy_w"]) == (list(range(n_vw)) if pairs else [])
    assert all(is_alt(v) for v in p["alt_w"]) and not any(is_alt(v) for v in p["copy_w"])
    if not (pairs or fkm):
        assert p["fc_perm"] == []
        return
    assert len(p["chunk"]) == (len(ch) if fkm else 0)
    for ci, (e0, e1) in enumerate(ch):
        w0, w1 = vfirst[e0], vfirst[e1]
        perm = p["fc_perm"][w0:w1]
        assert sorted(perm) == list(range(w0, w1))
        if not fkm:   # pair order: alt windows, stably by the SNV's place in the window's strand orientation
            def pos(v):
                q = c["var_pos"][c["win_seg"][v % n_win]] - c["win_off"][v % n_win]
                return 1999 - q if v >= rc_win else q
            na = sum(is_alt(v) for v in perm)
            alt, rest = perm[:na], perm[na:]
            assert all(is_alt(v) for v in alt) and not any(is_alt(v) for v in rest)
            assert [(pos(v), v) for v in alt] == sorted((pos(v), v) for v in alt)
            assert rest == sorted(rest)
            continue
        t = p["chunk"][ci]
        ws = list(zip(*[t["fk_ref"][k::4] for k in range(4)]))   # (w, block, conv6 offset, group start)
        assert [w[0] for w in ws] == perm
        assert sorted(t["fk_alt"]) == sorted(v for v in perm if is_alt(v)) and (pairs or not t["fk_alt"])
        n_ph = p["n_ph"][0]
        for v, b, off6, G in ws:   # a block belongs to one entry, so a group never mixes strands
            assert 0 <= b < (e1 - e0) * n_ph and e0 + b // n_ph == ent_of(v)
            assert 0 <= off6 - G <= 75 and (off6 - G) % 25 == 0
        groups = [list(g) for _, g in itertools.groupby(ws, key=lambda w: (w[1], w[3]))]
        assert len({(g[0][1], g[0][3]) for g in groups}) == len(groups)   # the windows of a group are contiguous
        galt = [any(is_alt(w[0]) for w in g) for g in groups]
        assert galt == sorted(galt, reverse=True)   # groups holding an alt window precede all others
        # gres per conv6 block: -2 unread, the groups' common start residue mod 100, else -1
        assert len(t["gres"]) == (e1 - e0) * n_ph
        for b, r in enumerate(t["gres"]):
            res = {g[0][3] % 100 for g in groups if g[0][1] == b}
            assert r == (-2 if not res else res.pop() if len(res) == 1 else -1)
        # slices: whole groups, <= fk_cap windows, in order; their alt-group prefix
        assert "slice_error" not in p
        bounds = {0}
        for g in groups:
            bounds.add(max(bounds) + len(g))
        sl = list(zip(*[t["slices"][k::4] for k in range(4)]))
        assert sl[0][0] == 0 and sl[-1][1] == len(ws) and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        for i0, i1, n_ag, nw_pre in sl:
            assert i0 in bounds and i1 in bounds and 0 < i1 - i0 <= c["fk_cap"]
            gs = [list(g) for _, g in itertools.groupby(ws[i0:i1], key=lambda w: (w[1], w[3]))]
            ga = [any(is_alt(w[0]) for w in g) for g in gs]
            assert n_ag == (ga + [False]).index(False) and nw_pre == sum(len(g) for g in gs[:n_ag])


def grid():
    cases = []
    k = 0
    for n_seg, n_per, step, mode, with_var in itertools.product(
            (1, 2, 3, 4), (1, 2, 3, 4, 5, 7, 10, 13, 20, 30), (200, 4), (FWD, RC, BOTH), (False, True)):
        win_seg, win_off, L = sweep(n_seg, n_per, step, uneven=True)
        proto = case(n_seg, L, mode, win_seg, win_off, 64)
        lo = max(min_max_batch(L, n_phases(proto)), n_phases(proto))
        var_pos = [(L // 2, 2, L - 3)[(s + n_per) % 3] for s in range(n_seg)] if with_var else None
        for merge, capped in itertools.product((0, 1), (False, True)):
            for mb in sorted({lo, lo + 1, (lo + 64) // 2, 64}):
                k += 1
                cases.append(case(n_seg, L, mode, win_seg, win_off, mb, var_pos=var_pos, merge=merge,
                                  chunk_windows=(n_per + n_per // 2) if capped else 0, fk=int(k % 4 != 0),
                                  fk_cap=(4, 9, FK_CAP)[k % 3]))
    return cases


def test_invariants(driver):
    cases = grid()
    seen = {"fkm pairs": 0, "pair order": 0, "slices": 0, "gres -1": 0, "chunks": 0}
    for c, p in zip(cases, plans(driver, cases)):
        check_plan(c, p)
        seen["fkm pairs"] += bool(p["fkm"][0]) and c["var_pos"] is not None and bool(p["alt_w"])
        seen["pair order"] += not p["fkm"][0] and bool(p["alt_w"]) and bool(p["copy_w"])
        seen["slices"] += any(len(t["slices"]) > 4 for t in p["chunk"])
        seen["gres -1"] += any(-1 in t["gres"] for t in p["chunk"])
        seen["chunks"] += len(p["chunks"]) > 2
    assert all(seen.values()), seen   # the grid reaches every branch the properties speak of


def strand_merge_case(n_shift, **kw):
    """3 SNVs on 200-bp sweeps of n_shift shifts, both strands, as tests/test_gpu_strand_merge.py runs
    them: one segment per SNV, the SNV at base 999 of the shift-0 window (pipeline.py: 999 - min shift)."""
    win_seg, win_off, L = sweep(3, n_shift, 200)
    return case(3, L, BOTH, win_seg, win_off, 64, var_pos=[200 * (n_shift // 2) + 999] * 3, **kw)


def test_pinned_chunk_lists(driver):
    for n in (20, 30):
        merged, knob0 = plans(driver, [strand_merge_case(n, chunk_windows=2 * n),
                                       strand_merge_case(n, chunk_windows=2 * n, merge=0)])
        assert merged["chunks"] == [0, 2, 2, 4, 4, 6]       # (fwd 0, fwd 1), (fwd 2, rc 0), (rc 1, rc 2)
        assert knob0["chunks"] == [0, 2, 2, 3, 3, 5, 5, 6]  # (f0, f1), (f2), (r0, r1), (r2)
        for c in (strand_merge_case(n, chunk_windows=2 * n), strand_merge_case(n)):
            check_plan(c, plans(driver, [c])[0])
        assert plans(driver, [strand_merge_case(n)])[0]["chunks"] == [0, 6]   # MAX_BATCH 64: one chunk


def test_pinned_fc1_mode(driver):
    """More than a third of the windows hold the SNV -> direct FC1 (10 and 20 shifts); 30: Karatsuba."""
    got = [bool(p["fkm"][0]) for p in plans(driver, [strand_merge_case(n) for n in (10, 20, 30)])]
    assert got == [False, False, True]
    alt = [len(p["alt_w"]) for p in plans(driver, [strand_merge_case(n) for n in (10, 20, 30)])]
    assert alt == [60, 60, 60]


@pytest.mark.parametrize("n_shift", [10, 20, 30])
def test_pinned_seg_cap(driver, n_shift):
    """The smallest max_batch of test_gpu_strand_merge.py's sweeps holds one segment, one less holds none."""
    c = strand_merge_case(n_shift)
    lo = min_max_batch(c["L"], 2)
    c["max_batch"] = max(lo, 2)
    c["p_cap"], c["q_cap"] = _caps(lo)
    ok, = plans(driver, [c])
    assert ok["n_ph"] == [2] and ok["seg_cap"] == [1] and ok["chunks"] == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    c["p_cap"], c["q_cap"] = _caps(lo - 1)
    assert plans(driver, [c])[0]["error"] == "segment too long for this handle's workspace (raise max_batch)"


def test_pinned_headline(driver):
    """bench.py's headline step: 96 SNVs x 200 shifts of 200 bp, both strands, max_batch 8192."""
    win_seg, win_off, L = sweep(96, 200, 200)
    assert L == 41800
    c = case(96, L, BOTH, win_seg, win_off, 8192, var_pos=[20999] * 96)
    p, = plans(driver, [c])
    assert p["seg_cap"] == [259]
    assert p["chunks"] == [0, 192]
    assert p["fkm"] == [1] and len(p["alt_w"]) == 2 * 96 * 10
    check_plan(c, p)


def test_refusals(driver):
    win_seg, win_off, L = sweep(2, 3, 200)
    base = dict(n_seg=2, L=L, mode=BOTH, win_seg=win_seg, win_off=win_off, max_batch=64)
    bad = {
        "windows must be sorted by segment": dict(base, win_seg=[0, 1, 0, 1, 1, 1]),
        "window segment out of range": dict(base, win_seg=[0, 0, 0, 1, 1, 2]),
        "window offset must be 4-aligned inside the segment": dict(base, win_off=[0, 202, 400, 0, 200, 400]),
        "window row out of range": dict(base, win_row=[0, 1, 2, 3, 4, 6]),
        "variant position outside its segment": dict(base, var_pos=[5, L]),
        "segment length must be >= 2000 and a multiple of 4": dict(base, L=L + 2),
        "segment too long for this handle's workspace (raise max_batch)": dict(base, caps=(10 ** 5, 10 ** 9)),
    }
    past = dict(base, win_off=[0, 200, L - 1996, 0, 200, 400])   # 4-aligned, but ends past the segment
    got = plans(driver, [case(**kw) for kw in list(bad.values()) + [past]])
    assert [p.get("error") for p in got] == list(bad) + ["window offset must be 4-aligned inside the segment"]
    # precedence, as forward_segments checked: the windows, then the workspace, then the pairs' tables
    both = dict(base, win_off=[0, 202, 400, 0, 200, 400], var_pos=[5, L], win_row=[9] * 6, caps=(10 ** 5, 10 ** 9))
    order = ["window offset must be 4-aligned inside the segment",
             "segment too long for this handle's workspace (raise max_batch)",
             "variant position outside its segment", "window row out of range"]
    for msg in order:
        assert plans(driver, [case(**both)])[0]["error"] == msg
        if msg == order[0]:
            both["win_off"] = base["win_off"]
        elif msg == order[1]:
            both.pop("caps")
        elif msg == order[2]:
            both["var_pos"] = [5, 6]
    # a window group larger than the Karatsuba slice is refused where the slice is cut
    # (8 shifts of 200 bp: the 4 windows of pool2 phase 0 are one group)
    win_seg, win_off, L = sweep(1, 8, 200)
    p, = plans(driver, [case(1, L, FWD, win_seg, win_off, 64, fk_cap=3)])
    assert p["slice_error"] == "a Karatsuba FC1 window group exceeds the FC1 slice"
