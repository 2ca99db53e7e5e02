"""The counts the shorter trip of the padded hydrogen-only march reached
(DESIGN_LOG.md 19), on the path tools/march_common_path.py reports - the same
listing and the same tool as tests/test_march_common_path.py, whose budgets
stay the older, wider ones.

The records hold sigma_H n x_H, so no build multiplies for a step's opacity:
one vector line fewer everywhere. The builds for packets of one weight (the
eighth flag of a PAD kernel) add path lengths and multiply at the flush: one
more. The first of the two dependent minima stands next to the key's select,
which took one of the two no-ops it would have cost on the scalar side."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "cmacionize_amd", "csrc")
LISTING = os.path.join(CSRC, "engine.s")

PLAIN = ("0", "0", "0", "0", "1", "0", "1")
HEAT = ("0", "1", "0", "0", "1", "0", "1")
# vector lines on the common path: a product per lane and step / path lengths
VECTOR_PER_LANE, VECTOR_UNIFORM, VECTOR_HEAT = 38, 37, 48
SCALAR_PLAIN, SCALAR_HEAT = 38, 39


@pytest.fixture(scope="module")
def listing():
    if not os.path.exists(LISTING):
        subprocess.run(["make", "-C", CSRC, "asm"], check=True)
    with open(LISTING) as f:
        return f.read().split("\n")


@pytest.fixture(scope="module")
def paths(listing):
    import march_common_path as m
    return {flags: m.counts(path) for flags, path in m.scan(listing).items()}


def test_all_six_padded_builds_are_there(paths):
    # <..., PAD, UNIFORM, BIG>
    assert sorted(f[7:] for f in paths if f[:7] == PLAIN) == [
        ("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")]
    assert sorted(f[7:] for f in paths if f[:7] == HEAT) == [
        ("0", "0"), ("0", "1")]
    assert len(paths) == 6


def test_vector_and_scalar_lines_of_the_trip(paths):
    for flags, c in paths.items():
        print(flags, c)
        if flags[:7] == HEAT:
            assert c["vector"] <= VECTOR_HEAT, (flags, c)
            assert c["scalar"] <= SCALAR_HEAT, (flags, c)
        else:
            uniform = flags[7] == "1"
            assert c["vector"] <= (VECTOR_UNIFORM if uniform
                                   else VECTOR_PER_LANE), (flags, c)
            assert c["scalar"] <= SCALAR_PLAIN, (flags, c)
        assert c["global"] == 1 and c["scratch"] == 0, (flags, c)
        assert c["readlane"] == 0, (flags, c)


def test_no_multiply_by_the_cross_section_and_none_by_the_weight(listing):
    """Double-precision multiplies on the path: the step's optical depth
    (ds x record) in every build, the weighed path length where weights
    differ, the heating term's."""
    import march_common_path as m
    for flags, path in m.scan(listing).items():
        muls = sum(t.startswith("v_mul_f64") for t in path)
        want = 3 if flags[:7] == HEAT else (1 if flags[7] == "1" else 2)
        assert muls == want, (flags, muls)


def test_plain_builds_keep_64_registers_and_8_waves(listing):
    import march_common_path as m
    found = 0
    for i, line in enumerate(listing):
        k = m.KERNEL.match(line)
        if not k:
            continue
        flags = tuple(re.findall(r"Lb([01])E", k.group(1)))
        if flags[:7] != PLAIN:
            continue
        tail = "\n".join(listing[i:i + 20000])
        vgprs = int(re.search(r"^; NumVgprs: (\d+)", tail, re.M).group(1))
        waves = int(re.search(r"^; Occupancy: (\d+)", tail, re.M).group(1))
        print(flags, vgprs, waves)
        assert vgprs <= 64 and waves == 8, (flags, vgprs, waves)
        found += 1
    assert found == 4
