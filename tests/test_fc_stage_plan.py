"""The alt rows the segment planner (expecto_amd/csrc/seg_plan.h, SegPlan::fk_alt_plan) gives a
Karatsuba FC1 slice of segment pairs, without a GPU: tests/fc_stage_plan_driver.cpp prints them and
they are set against a brute-force statement of the rule -- an alt group's partial (product, K slab)
is recomputed iff an alt window of the group sums that product and a row the partial reads, through
its sequence's lags, is a changed conv6 row of its block; an alt window's tail iff one of its rows
100..105 is.  The SNV is swept across a whole group's 175-row span (and both segment ends).  The
driver also runs once under the address and undefined-behaviour sanitizers.  Last, what the handle's
knob parser makes of the stage's two settings (tests/fc_stage_switch_driver.cpp)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fc_stage_plan_driver.cpp")
FWD, RC, BOTH = 0, 1, 2

# DESIGN.md "FC1 as a block-Karatsuba convolution": product g reads block BLK[g] of its group from the
# sequence with lags LAGS[g] (X: none; D1[r] = x[r] - x[r+25]; D2: 50; DD: 25, 50, 75); role a sums ROLE[a]
BLK = [0, 1, 1, 2, 3, 3, 2, 3, 3]
LAGS = [(0, 25, 50, 75), (0, 50), (0, 25, 50, 75), (0, 25), (0,), (0, 25), (0, 25, 50, 75), (0, 50), (0, 25, 50, 75)]
ROLE = [(0, 1, 3, 4), (1, 2, 4, 5), (3, 4, 6, 7), (4, 5, 7, 8)]
W6 = 20   # changed conv6 rows per block: [r6, r6 + 20)


def _cxx():
    return [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fc_stage_plan") / "fc_stage_plan_driver")
    subprocess.run(_cxx() + ["-std=c++17", "-O1", "-Wall", SRC, "-o", exe], check=True)
    return exe


def case(n_seg, n_shift, mode, var_pos, max_batch=64, fk_cap=10 ** 6, inplace=0, drop=()):
    """n_shift windows at 200 bp per segment, less the shifts in `drop`."""
    js = [j for j in range(n_shift) if j not in drop]
    win_seg = [s for s in range(n_seg) for _ in js]
    win_off = [200 * j for _ in range(n_seg) for j in js]
    L = 2000 + 200 * (n_shift - 1)
    return dict(head=[n_seg, L, mode, len(win_seg), max_batch, fk_cap, inplace], win_seg=win_seg, win_off=win_off,
                var_pos=list(var_pos))


def plans(exe, cases):
    text = "\n".join(" ".join(map(str, c["head"] + c["win_seg"] + c["win_off"] + c["var_pos"])) for c in cases) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    res, cur = [], None
    for ln in out.splitlines():
        name, _, rest = ln.partition(" ")
        if name == "case":
            cur = {"slices": []}
        elif name == "end":
            res.append(cur)
        elif name == "error":
            cur["error"] = rest
        else:
            v = [int(x) for x in rest.split()]
            if name == "slice":
                cur["slices"].append({"head": v, "win": [], "grp": {}})
            elif name == "win":
                cur["slices"][-1]["win"].append(v)
            elif name == "grp":
                cur["slices"][-1]["grp"][(v[0], v[1])] = v[2:]
            elif name in ("alt", "tail"):
                cur["slices"][-1][name] = v
            else:
                cur[name] = v
    assert len(res) == len(cases)
    return res


def slab_rows(s):
    """Rows of a 25-row block whose K elements (640 per row) meet slab s of 8000."""
    return range(8000 * s // 640, (8000 * (s + 1) - 1) // 640 + 1)


def reached(G, g, s, r6):
    changed = np.zeros(4096, bool)
    changed[r6:r6 + W6] = True
    rows = np.array([G + 25 * BLK[g] + i + lag for i in slab_rows(s) for lag in LAGS[g]])
    return bool(changed[rows].any())


def check_slice(sl, fk_cap, inplace):
    """The slice's alt rows against the brute-force rule; returns what it saw."""
    ci, i0, i1, n_ag, nw_pre = sl["head"]
    win = sl["win"]
    assert len(win) == i1 - i0
    groups = [list(g) for _, g in itertools.groupby(enumerate(win), key=lambda t: (t[1][1], t[1][2] - 25 * (t[1][2] // 25 % 4)))]
    galt = [any(w[3] for _, w in g) for g in groups]
    assert n_ag == (galt + [False]).index(False) and nw_pre == sum(len(g) for g in groups[:n_ag])
    assert not any(galt[n_ag:])   # every alt window of a slice is in its leading alt groups
    n_alt = sum(w[3] for w in win)
    assert len(win) + (0 if inplace else n_alt) <= fk_cap or len(groups) == 1
    seen = {"reached": 0, "kept": 0, "tail": 0, "no tail": 0, "sparse": 0}
    if n_ag == 0:
        assert "alt" not in sl
        return seen
    assert sl["alt"] == [i for i, w in enumerate(win) if w[3]]
    want_tail = [i for i, w in enumerate(win) if w[3] and any(w[4] <= w[2] + r < w[4] + W6 for r in range(100, 106))]
    assert sl["tail"] == want_tail
    seen["tail"] += len(want_tail)
    seen["no tail"] += n_alt - len(want_tail)
    for g, s in itertools.product(range(9), range(2)):
        want = []
        for k, grp in enumerate(groups[:n_ag]):
            G = grp[0][1][2] - 25 * (grp[0][1][2] // 25 % 4)
            summed = any(w[3] and g in ROLE[(w[2] - G) // 25] for _, w in grp)
            hit = reached(G, g, s, grp[0][1][4])
            if summed and hit:
                want.append(k)
            seen["reached"] += summed and hit
            seen["kept"] += summed and not hit
            seen["sparse"] += hit and not summed
        assert sl["grp"][(g, s)] == want, (g, s)
    return seen


def sweep_cases():
    """The SNV at every 8th base of a stretch longer than a group's span (175 conv6 rows = 2800 bases),
    and at both ends of the segment (clamped runs); 60 shifts, so a third or fewer windows are alt."""
    n_shift, L = 60, 2000 + 200 * 59
    pos = list(range(5000, 5000 + 3000, 8)) + [0, 1, 7, 500, L - 501, L - 2, L - 1]
    return [case(1, n_shift, mode, [q]) for q in pos for mode in (FWD, BOTH)]


def test_alt_rows_match_the_brute_force_rule(driver):
    cases = sweep_cases()
    total = {}
    for c, p in zip(cases, plans(driver, cases)):
        assert "error" not in p and p["fkm"] == [1], c["var_pos"]
        assert len(p["slices"]) == 1   # one chunk, one slice
        for sl in p["slices"]:
            for k, v in check_slice(sl, c["head"][5], 0).items():
                total[k] = total.get(k, 0) + v
    assert all(total[k] for k in ("reached", "kept", "tail", "no tail")), total


def test_sparse_groups_and_slices(driver):
    """Groups of 1-3 windows (dropped shifts), several segments and slices under a small cap: an alt
    window counts twice towards the cap unless the alt pass runs in place."""
    drop = tuple(j for j in range(60) if j % 7 in (2, 3) or j in (29, 31))
    cases = [case(3, 60, BOTH, [5999, 6400, 7000], fk_cap=cap, inplace=ip, drop=drop)
             for cap in (24, 64, 10 ** 6) for ip in (0, 1)]
    total = {}
    for c, p in zip(cases, plans(driver, cases)):
        assert "error" not in p and p["fkm"] == [1]
        with_alt = 0
        for sl in p["slices"]:
            for k, v in check_slice(sl, c["head"][5], c["head"][6]).items():
                total[k] = total.get(k, 0) + v
            with_alt += sl["head"][3] > 0
        if c["head"][5] == 24:
            assert with_alt >= 2   # alt groups in more than one slice
        windows = sorted(w[0] for sl in p["slices"] for w in sl["win"])
        assert windows == list(range(2 * len(c["win_seg"])))
    assert total["sparse"] and total["reached"] and total["kept"], total


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fc_stage_plan_driver_san")
    subprocess.run(_cxx() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                             "-o", exe], check=True)
    cases = sweep_cases()[::40] + [case(3, 60, BOTH, [5999, 6400, 7000], fk_cap=24, drop=(2, 3, 9, 10, 29, 31))]
    for p in plans(exe, cases):
        assert "error" not in p and p["slices"]


def test_switch_and_slice_default(tmp_path):
    """EXPECTO_FC1K_ALT_INPLACE is off unless set to a nonzero integer; the slice cap defaults to 0 (auto:
    a multiple of max_batch) and EXPECTO_FC1K_SLICE sets it."""
    exe = str(tmp_path / "fc_stage_switch_driver")
    subprocess.run(_cxx() + ["-std=c++17", "-O1", "-Wall", os.path.join(REPO, "tests", "fc_stage_switch_driver.cpp"),
                             "-o", exe], check=True)
    run = lambda *kv: subprocess.run([exe, *kv], capture_output=True, text=True, check=True).stdout.split()
    assert run() == ["fk_slice", "0", "fk_alt_inplace", "0"]
    assert run("EXPECTO_FC1K_ALT_INPLACE=1") == ["fk_slice", "0", "fk_alt_inplace", "1"]
    assert run("EXPECTO_FC1K_ALT_INPLACE=0", "EXPECTO_FC1K_SLICE=700") == ["fk_slice", "700", "fk_alt_inplace", "0"]
    assert run("EXPECTO_FC1K_ALT_INPLACE=1", "EXPECTO_FC1_ROLE=9")[0] == "error"
