"""The handle's EXPECTO_* knobs (expecto_amd/csrc/beluga_knobs.h), without a GPU: the header is built
with the host compiler alone into tests/beluga_knobs_driver.cpp, which prints every knob's field for
each environment it reads.  The knob names and defaults come from INTEGRATION.md's table, so a knob
in the document without a table entry in the header (or the reverse) fails here."""
import math
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a value other than the default for every knob that is not an on/off flag
VALUES = {
    "EXPECTO_CONV_TILE": "384", "EXPECTO_FC1_SPLITS": "4", "EXPECTO_FC2_SPLITS": "9", "EXPECTO_FC2_ROWS": "12345",
    "EXPECTO_SEG_CHUNK_WINDOWS": "77", "EXPECTO_FC1_M_ORDER_MB": "12.5", "EXPECTO_FC1_ORDER": "2",
    "EXPECTO_FC1_M_GROUP": "4", "EXPECTO_KMER_MAX_BYTES": "10737418240", "EXPECTO_FC1_ROLE": "2",
    "EXPECTO_FC1K_SLICE": "1000", "EXPECTO_FC1_NARROW": "1", "EXPECTO_CONV_NARROW": "0",
}


def documented():
    """{variable: default} of the knobs expecto_beluga_create reads, from INTEGRATION.md's table (the rows
    marked (Python) are read by the Python package).  'unset' is no cap (inf); EXPECTO_FC2_ROWS' default
    is derived from max_batch at creation, its raw value is 0."""
    rows = {}
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        for ln in f:
            m = re.match(r"\| `(EXPECTO_\w+)`( \(Python\))? \| ([^|]*) \|", ln)
            if m and not m.group(2):
                d = m.group(3).strip()
                num = re.match(r"-?\d+", d)
                rows[m.group(1)] = 0.0 if m.group(1) == "EXPECTO_FC2_ROWS" else math.inf if d == "unset" else float(num.group())
    return rows


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("beluga_knobs") / "beluga_knobs_driver")
    cxx = [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", os.path.join(REPO, "tests", "beluga_knobs_driver.cpp"), "-o", exe],
                   check=True)
    return exe


def parse(driver, envs):
    """Per environment (a dict) {variable: field value}, or {'error': refusal}."""
    text = "".join(" ".join(f"{k}={v}" for k, v in e.items()) + "\n" for e in envs)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout
    res, cur = [], None
    for ln in out.splitlines():
        name, _, rest = ln.partition(" ")
        if name == "case":
            cur = {}
        elif name == "end":
            res.append(cur)
        else:
            cur[name] = rest if name == "error" else float(rest)
    assert len(res) == len(envs)
    return res


def test_the_document_lists_the_knobs():
    doc = documented()
    assert len(doc) == 25 and set(VALUES) <= set(doc), sorted(doc)


def test_empty_environment_gives_the_documented_defaults(driver):
    got, = parse(driver, [{}])
    assert got == documented()


def test_each_knob_changes_its_field_and_no_other(driver):
    doc = documented()
    names = sorted(doc)
    envs = [{n: VALUES.get(n, "0" if doc[n] else "1")} for n in names]
    for n, env, got in zip(names, envs, parse(driver, envs)):
        want = dict(doc)
        want[n] = float(env[n])
        assert want[n] != doc[n] and got == want, n


def test_accepted_ranges(driver):
    """Every value a constrained knob accepts, and on/off flags from any integer (atoi != 0)."""
    cases = [("EXPECTO_FC1_SPLITS", v, v) for v in (1, 2, 4, 5, 8, 10, 20)]
    cases += [("EXPECTO_FC2_SPLITS", v, v) for v in (1, 3, 7, 9, 21, 63)]
    cases += [("EXPECTO_FC1_ROLE", v, v) for v in range(5)]
    cases += [(k, v, v) for k in ("EXPECTO_CONV_NARROW", "EXPECTO_FC1_NARROW") for v in (-1, 0, 1)]
    cases += [("EXPECTO_CONV_TILE", v, v) for v in (0, 256, 384)]
    cases += [("EXPECTO_FC_WIDE", "2", 1), ("EXPECTO_FC_WIDE", "-1", 1), ("EXPECTO_FC_WIDE", "off", 0),
              ("EXPECTO_SEG_CHUNK_WINDOWS", "-3", -3), ("EXPECTO_FC1_M_ORDER_MB", "0.5", 0.5)]
    got = parse(driver, [{k: v} for k, v, _ in cases])
    for (k, v, want), g in zip(cases, got):
        assert g.get(k) == want, (k, v, g)


REFUSALS = [
    ("EXPECTO_FC1_SPLITS", "33", "EXPECTO_FC1_SPLITS must divide 2120 and be <= 32"),
    ("EXPECTO_FC1_SPLITS", "7", "EXPECTO_FC1_SPLITS must divide 2120 and be <= 32"),
    ("EXPECTO_FC1_SPLITS", "0", "EXPECTO_FC1_SPLITS must divide 2120 and be <= 32"),
    ("EXPECTO_FC1_SPLITS", "40", "EXPECTO_FC1_SPLITS must divide 2120 and be <= 32"),   # a divisor above 32
    ("EXPECTO_FC2_SPLITS", "0", "EXPECTO_FC2_SPLITS must divide 63"),
    ("EXPECTO_FC2_SPLITS", "2", "EXPECTO_FC2_SPLITS must divide 63"),
    ("EXPECTO_FC1_ROLE", "5", "EXPECTO_FC1_ROLE must be 0..4"),
    ("EXPECTO_FC1_ROLE", "-1", "EXPECTO_FC1_ROLE must be 0..4"),
    ("EXPECTO_CONV_NARROW", "2", "EXPECTO_CONV_NARROW must be -1 (auto), 0 or 1"),
    ("EXPECTO_FC1_NARROW", "-2", "EXPECTO_FC1_NARROW must be -1 (auto), 0 or 1"),
    ("EXPECTO_CONV_TILE", "128", "EXPECTO_CONV_TILE must be 0 (auto), 256 or 384"),
]


def test_refusals(driver):
    got = parse(driver, [{k: v} for k, v, _ in REFUSALS])
    assert [g.get("error") for g in got] == [t for _, _, t in REFUSALS]
    # a refused knob refuses whatever else is set
    got, = parse(driver, [{"EXPECTO_FC_WIDE": "0", "EXPECTO_CONV_TILE": "128", "EXPECTO_OVERLAP": "0"}])
    assert got == {"error": "EXPECTO_CONV_TILE must be 0 (auto), 256 or 384"}


def test_clamps(driver):
    """Values below 1 are raised to 1, not refused."""
    cases = [("EXPECTO_FC1_M_GROUP", "0"), ("EXPECTO_FC1K_SLICE", "-5"), ("EXPECTO_FC2_ROWS", "0")]
    got = parse(driver, [{k: v} for k, v in cases])
    assert [g.get(k) for (k, _), g in zip(cases, got)] == [1, 1, 1]
