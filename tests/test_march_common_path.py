"""Guard on the common path of the padded hydrogen-only march loop.

The loop is bound by instruction issue: a SIMD issues one
vector and one scalar instruction per four cycles, so a wave trip is as long
as the larger of the two counts, and the kernel's time follows them.
tools/march_common_path.py extracts the path nearly every trip takes - loop
header to the "every lane found its table slot" branch after the first
ds_add_f64, without the end-of-flight block, and back to the header - from the
compiler's listing. Before the loop was shortened the tool counted 45 vector
and 61 scalar lines on it (scalar: no-ops, waits and branches included); the
budgets are those counts less the 5 and 8 the shortening had to deliver at the
least. A spill or a v_readlane on the path costs far more than an instruction
(DESIGN_LOG.md 4.1): none is allowed, in the heating builds either."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "cmacionize_amd", "csrc")
LISTING = os.path.join(CSRC, "engine.s")

PARENT_VECTOR, PARENT_SCALAR = 45, 61
VECTOR_BUDGET = PARENT_VECTOR - 5
SCALAR_BUDGET = PARENT_SCALAR - 8


@pytest.fixture(scope="module")
def paths():
    if not os.path.exists(LISTING):
        subprocess.run(["make", "-C", CSRC, "asm"], check=True)
    import march_common_path as m
    with open(LISTING) as f:
        found = m.scan(f.read().split("\n"))
    return {flags: (path, m.counts(path)) for flags, path in found.items()}


def test_tool_finds_the_benchmark_kernels(paths):
    # <FULL, HEAT, REEMIT, EXACT, TABLE, PRE, PAD, ...>: hydrogen only, table,
    # padded records - without and with the heating term
    plain = [f for f in paths if f[:7] == ("0", "0", "0", "0", "1", "0", "1")]
    heat = [f for f in paths if f[:7] == ("0", "1", "0", "0", "1", "0", "1")]
    assert plain and heat, sorted(paths)
    for flags, (path, c) in paths.items():
        # the path is the march: the record's load, the table's compare-and-
        # swap and add, the three selects' rounds of the run sums
        assert c["global"] == 1, (flags, c)
        assert c["lds"] >= 2, (flags, c)
        assert any(t.startswith("ds_cmpst") for t in path), flags
        assert sum("v_cndmask_b32_dpp" in t for t in path) >= 6, flags
        assert not any("v_rcp_f64" in t for t in path), flags


def test_no_spill_and_no_readlane_on_the_common_path(paths):
    for flags, (path, c) in paths.items():
        print(flags, c)
        assert c["scratch"] == 0, (flags, c)
        assert c["readlane"] == 0, (flags, c)


def test_common_path_instruction_budgets(paths):
    plain = {f: c for f, (_, c) in paths.items()
             if f[:7] == ("0", "0", "0", "0", "1", "0", "1")}
    assert plain
    for flags, c in plain.items():
        print(flags, c)
        assert c["vector"] <= VECTOR_BUDGET, (flags, c)
        assert c["scalar"] <= SCALAR_BUDGET, (flags, c)
