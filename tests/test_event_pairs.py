"""The profiling timers' event-pair bookkeeping (expecto_amd/csrc/event_pairs.h), without a GPU: the
header is built with the host compiler alone into tests/event_pairs_driver.cpp, which runs scripted
open / close sequences the way beluga.hip's Timer does and prints every event.  The rules checked on
each log: a pair is never handed out while it is open or closed but not yet read; a resolve happens
only with no timer open; the pool grows by no more than the timers open at that moment; every closed
timer is read exactly once, with its own pair."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 8

LAYER = ["L", "c"]                    # a layer's launches in its slot's timer
CONV = ["L", "G", "c", "c"]           # run_conv: the GEMM launch's own timer inside the layer's


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("event_pairs") / "event_pairs_driver")
    cxx = [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", os.path.join(REPO, "tests", "event_pairs_driver.cpp"), "-o", exe],
                   check=True)
    return exe


def run(driver, scripts, pairs=PAIRS):
    text = "".join(" ".join([str(pairs)] + ops) + "\n" for ops in scripts)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout
    logs, cur = [], None
    for ln in out.splitlines():
        if ln == "case":
            cur = []
        elif ln == "end":
            logs.append(cur)
        else:
            cur.append(ln.split())
    assert len(logs) == len(scripts)
    return logs


def check(ops, log, pairs=PAIRS):
    """The rules above on one log; returns (resolves, final capacity, wraps): wraps lists, per timer that
    opened on a full pool, (its serial, 'resolve' or 'grow').  The script ends with an R."""
    assert ops[-1] == "R"
    kind = {}                      # serial -> 'layer' / 'launch', from the script
    for op in ops:
        if op in "LG":
            kind[len(kind)] = "layer" if op == "L" else "launch"
    cap, open_, pending, read = pairs, {}, {}, {}
    resolves, i, wraps = 0, 0, []
    while i < len(log):
        ev = log[i]
        i += 1
        if ev[0] == "open":
            serial, pair = int(ev[1]), int(ev[2])
            assert 0 <= pair < cap, ev
            assert pair not in open_.values() and pair not in pending.values(), ("pair handed out twice", ev)
            open_[serial] = pair
        elif ev[0] == "close":
            serial, pair = int(ev[1]), int(ev[2])
            assert open_.pop(serial) == pair
            pending[serial] = pair
        elif ev[0] == "grow":
            n_open, after = int(ev[1]), int(ev[2])
            assert n_open == len(open_) and 0 < after - cap <= n_open, ev
            cap = after
            wraps.append((int(log[i][1]), "grow"))
        else:
            assert ev[0] == "resolve" and int(ev[1]) == 0 and not open_, ("resolve with a timer open", ev)
            resolves += 1
            got = {}
            while i < len(log) and log[i][0] == "sample":
                assert log[i][1] == kind[int(log[i][2])], log[i]
                assert int(log[i][2]) not in got and int(log[i][2]) not in read, ("read twice", log[i])
                got[int(log[i][2])] = int(log[i][3])
                i += 1
            assert got == pending, "a resolve reads every closed timer with its own pair"
            read.update(got)
            pending = {}
            if i < len(log):
                wraps.append((int(log[i][1]), "resolve"))
    assert not open_ and not pending and sorted(read) == list(range(len(kind)))
    return resolves, cap, wraps


def test_depth_1_wraps(driver):
    ops = LAYER * (5 * PAIRS + 3) + ["R"]
    (log,) = run(driver, [ops])
    resolves, cap, _ = check(ops, log)
    assert resolves == 6 and cap == PAIRS      # 5 wraps and the last R; never grown


def test_depth_2_wraps_at_every_phase(driver):
    """A call of 7 pairs (conv1, conv2 .. conv3 with their launch timers, the FC layers) after k single
    layers, k = 0 .. 7: over 6 calls the 8-pair pool wraps at least three times, and over the k the
    wrap lands on each of the call's 7 timers: a launch timer (the call's timers 2 and 4) grows the
    pool, a layer timer resolves it."""
    call = LAYER + CONV + CONV + LAYER + LAYER
    scripts = [LAYER * k + call * 6 + ["R"] for k in range(PAIRS)]
    seen = set()
    for k, (ops, log) in enumerate(zip(scripts, run(driver, scripts))):
        resolves, cap, wraps = check(ops, log)
        assert resolves >= 4 and len(wraps) >= 3, (resolves, wraps)
        seen |= {((serial - k) % 7, how) for serial, how in wraps if serial >= k}
    assert seen == {(0, "resolve"), (1, "resolve"), (2, "grow"), (3, "resolve"), (4, "grow"), (5, "resolve"),
                    (6, "resolve")}


def test_layer_at_the_last_pair_launch_on_a_full_pool(driver):
    """The sequence that used to hand the open layer timer's pair out again: the layer timer takes the
    pool's last pair, its launch timer opens on a full pool.  The pool grows by one pair, nothing is
    resolved until both are closed, and the next timer's resolve reads both with their own pairs."""
    ops = LAYER * (PAIRS - 1) + CONV + LAYER + ["R"]
    (log,) = run(driver, [ops])
    check(ops, log)
    tail = log[2 * (PAIRS - 1):]
    assert tail[:5] == [["open", "7", "7"], ["grow", "1", "9"], ["open", "8", "8"], ["close", "8", "8"],
                        ["close", "7", "7"]]
    assert tail[5] == ["resolve", "0"]
    assert ["sample", "layer", "7", "7"] in tail and ["sample", "launch", "8", "8"] in tail
    assert tail[5 + 1 + PAIRS + 1] == ["open", "9", "0"]


def test_outside_resolve_between_calls(driver):
    """layer_times / main_launches resolve between calls (no timer open): the pairs start again at 0."""
    ops = CONV + ["R"] + CONV + ["R"]
    (log,) = run(driver, [ops])
    check(ops, log)
    assert [ev[2] for ev in log if ev[0] == "open"] == ["0", "1", "0", "1"]
