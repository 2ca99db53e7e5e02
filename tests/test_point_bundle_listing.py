"""Guard on the listing of the point build of the bundle kernel
(shoot_bundle_kernel<true, true>), in the style of
test_bundle_listing.py; skipped without the compiler's listing
(`make -C cmacionize_amd/csrc asm`).

The point build shares the march loop's text with the bundle build
shoot_bundle_kernel<true> and is compared with it in the same listing: the
same common path (37 vector / 38 scalar lines, no scratch access, no lane
move), 64 VGPRs, and - what it is for - less of everything the bundle build
carries around the march: strictly fewer SGPR spills, VGPR spills and scratch
bytes, strictly fewer lane moves and vector lines in the outer loop outside
the march, and one copy of random_direction (one v_trig_preop_f64 triple)
where the bundle build holds three."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LISTING = os.path.join(ROOT, "cmacionize_amd", "csrc", "engine.s")

BOUND = (37, 38)
BUNDLE = "_Z19shoot_bundle_kernelILb1EEv9ShootArgs"
POINT = "_Z19shoot_bundle_kernelILb1ELb1EEv9ShootArgsPK12PointEmitDev"


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(LISTING):
        pytest.skip("no listing: make -C cmacionize_amd/csrc asm")
    import bundle_outer_loop as b
    return b


@pytest.fixture(scope="module")
def text(tool):
    with open(LISTING) as f:
        return f.read().split("\n")


@pytest.fixture(scope="module")
def listing(tool, text):
    return tool.report(text)


def outer_lines(tool, text, symbol):
    """the instructions of the kernel's outer loop, the march loop included"""
    import march_common_path as mcp
    body = tool.kernel_bodies(text)[symbol]
    inner, outer = tool.outer_loop(body)
    assert inner is not None and outer is not None
    oh, oe = outer
    return [t for _, t in mcp.instructions(body[oh:oe + 1])]


def test_point_build_is_in_the_code_object(listing):
    assert POINT in listing and BUNDLE in listing, sorted(listing)
    r = listing[POINT]
    assert r["common"] is not None and r["outer"] is not None
    # the path is the march: one record load, the table's compare-and-swap
    # and add
    assert r["common"]["global"] == 1
    assert any(t.startswith("ds_cmpst") for t in r["path"])
    assert any(t.startswith("ds_add_f64") for t in r["path"])


def test_common_path_of_the_point_build(listing):
    c = listing[POINT]["common"]
    print("point", c, "bundle", listing[BUNDLE]["common"])
    assert c["scratch"] == 0
    assert c["readlane"] == 0
    assert c["vector"] <= BOUND[0]
    assert c["scalar"] <= BOUND[1]


def test_registers_spills_and_scratch_of_the_point_build(listing):
    new = listing[POINT]["resources"]
    old = listing[BUNDLE]["resources"]
    print("point", new)
    print("bundle", old)
    assert new["vgpr_count"] == 64
    assert new["sgpr_spill_count"] < old["sgpr_spill_count"]
    assert new["vgpr_spill_count"] < old["vgpr_spill_count"]
    assert new["private_segment_fixed_size"] < \
        old["private_segment_fixed_size"]


def test_outer_loop_of_the_point_build(listing):
    new = listing[POINT]["outer"]
    old = listing[BUNDLE]["outer"]
    print("point", new)
    print("bundle", old)
    assert new["lane_moves"] < old["lane_moves"]
    assert new["vector"] < old["vector"]


def test_one_copy_of_random_direction(tool, text):
    """sincos of an fp64 argument reduces it with three v_trig_preop_f64: a
    triple per inlined copy of random_direction."""
    new = sum(t.startswith("v_trig_preop_f64")
              for t in outer_lines(tool, text, POINT))
    old = sum(t.startswith("v_trig_preop_f64")
              for t in outer_lines(tool, text, BUNDLE))
    print("v_trig_preop_f64: point", new, "bundle", old)
    assert new == 3
