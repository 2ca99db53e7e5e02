"""Guard on the listing of the bundle builds of the padded first generation
(shoot_bundle_kernel<UNIFORM>), in the style of
test_march_common_path.py; skipped without the compiler's listing
(`make -C cmacionize_amd/csrc asm`).

The bundle builds share the march loop's text with the general builds, and a
wave trip costs what the longer of its vector and scalar counts costs. The
UNIFORM build - the headline run's - stays within 37 vector and 38 scalar lines
on the common path, the general UNIFORM build's counts. The build with a
product per lane forms that product on the path, one vector line more, as the
general build of that weight does (38 / 38): its bound is 38 / 38. Neither has
scratch accesses or lane moves on the path; the kernels keep 64 VGPRs (8 waves
per SIMD) and need no more scratch per lane than the general build of the same
weight.

(With the packet counts held in scalar registers across the march the
per-lane build's path was 38 / 39; they wait in LDS for that reason,
DESIGN_LOG.md 21.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LISTING = os.path.join(ROOT, "cmacionize_amd", "csrc", "engine.s")

# {UNIFORM: (vector, scalar)}
BOUNDS = {1: (37, 38), 0: (38, 38)}
BUNDLE = "_Z19shoot_bundle_kernelILb%dEEv9ShootArgs"
GENERAL = "_Z12shoot_kernelILb0ELb0ELb0ELb0ELb1ELb0ELb1ELb%dELb0EEv9ShootArgs"


@pytest.fixture(scope="module")
def listing():
    if not os.path.exists(LISTING):
        pytest.skip("no listing: make -C cmacionize_amd/csrc asm")
    import bundle_outer_loop as b
    with open(LISTING) as f:
        return b.report(f.read().split("\n"))


def test_both_bundle_builds_are_in_the_code_object(listing):
    for uniform in (0, 1):
        assert BUNDLE % uniform in listing, sorted(listing)
        assert GENERAL % uniform in listing, sorted(listing)
        r = listing[BUNDLE % uniform]
        assert r["common"] is not None and r["outer"] is not None
        # the path is the march: one record load, the table's compare-and-
        # swap and add
        assert r["common"]["global"] == 1
        assert any(t.startswith("ds_cmpst") for t in r["path"])
        assert any(t.startswith("ds_add_f64") for t in r["path"])


@pytest.mark.parametrize("uniform", [1, 0])
def test_common_path_of_the_bundle_build(listing, uniform):
    c = listing[BUNDLE % uniform]["common"]
    print("bundle", uniform, c, "general",
          listing[GENERAL % uniform]["common"])
    assert c["scratch"] == 0
    assert c["readlane"] == 0
    assert c["vector"] <= BOUNDS[uniform][0]
    assert c["scalar"] <= BOUNDS[uniform][1]


@pytest.mark.parametrize("uniform", [1, 0])
def test_registers_and_scratch_of_the_bundle_build(listing, uniform):
    new = listing[BUNDLE % uniform]
    old = listing[GENERAL % uniform]
    print("bundle", uniform, new["resources"], new["outer"])
    print("general", uniform, old["resources"], old["outer"])
    assert new["resources"]["vgpr_count"] == 64
    assert new["resources"]["private_segment_fixed_size"] <= \
        old["resources"]["private_segment_fixed_size"]
