"""The bucket order's plan (cmacionize_amd/csrc/packet_order_plan.h): the bits
of the two scatter levels, the capacities of a region and a leaf and their
places in the sort buffers, for launches of 1 to 2^27 packets. The planner is
a plain host function; a small stand-alone program calls it."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "cmacionize_amd", "csrc")

PROGRAM = r"""
#include "packet_order_plan.h"
#include <cstdio>
int main() {
  unsigned long long n, min_packets;
  int key_bits, bits1, bits2, slack;
  while (std::scanf("%llu %d %d %d %d %llu", &n, &key_bits, &bits1, &bits2,
                    &slack, &min_packets) == 6) {
    const BucketPlan b = cmi_bucket_plan(n, key_bits, bits1, bits2, slack,
                                         min_packets);
    std::printf("%d %d %d %d %u %u %llu %llu %llu %llu\n", b.take, b.bits1,
                b.bits2, b.rem_bits, b.region_cap, b.leaf_cap,
                (unsigned long long)b.region_begin,
                (unsigned long long)b.region_words,
                (unsigned long long)b.leaf_begin,
                (unsigned long long)b.total_words);
  }
  std::printf("limits %d %d %d %d\n", CMI_BUCKET_LEVEL_BITS,
              CMI_BUCKET_REM_BITS, CMI_BUCKET_LEAF_PAIRS,
              CMI_BUCKET_TIE_PAIRS);
  return 0;
}
"""

# what the leaf kernel keeps in LDS per pair (the id by bin, the ordered id)
# and for its bins, against the 64 KB a workgroup may have
LDS_BYTES_PER_PAIR = 8
LDS_BYTES_BINS = 2048
LDS_BUDGET = 64 << 10


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = (os.environ.get("CXX") or shutil.which("c++") or
           shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no C++ compiler for the stand-alone planner program"
    d = tmp_path_factory.mktemp("packet_order_plan")
    src = d / "plan.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I", HEADER_DIR, "-o", str(exe), str(src)], check=True)

    def run(cases):
        text = "".join("%d %d %d %d %d %d\n" % c for c in cases)
        out = subprocess.run([str(exe)], input=text, capture_output=True,
                             text=True, check=True).stdout.split("\n")
        assert out[len(cases)].startswith("limits")
        limits = tuple(int(x) for x in out[len(cases)].split()[1:])
        keys = ("take", "bits1", "bits2", "rem", "region_cap", "leaf_cap",
                "region_begin", "region_words", "leaf_begin", "total_words")
        plans = [dict(zip(keys, (int(x) for x in line.split())))
                 for line in out[:len(cases)]]
        return plans, limits
    return run


def counts():
    """1 .. 2^27: around every power of two, and a few thousand others."""
    ns = {1, 2, 3, 100000000, 10000000, 1000000}
    for k in range(1, 28):
        ns.update((2 ** k - 1, 2 ** k, 2 ** k + 1))
    rng = np.random.default_rng(5)
    ns.update(int(x) for x in np.exp(rng.uniform(0., math.log(2. ** 27),
                                                 3000)).astype(np.int64))
    return sorted(n for n in ns if 1 <= n <= 2 ** 27)


def check_taken(n, key_bits, slack, b, limits):
    level_bits, rem_bits, leaf_pairs, tie_pairs = limits
    assert 0 <= b["bits1"] <= level_bits and 0 <= b["bits2"] <= level_bits
    assert b["rem"] == key_bits - b["bits1"] - b["bits2"]
    assert 0 <= b["rem"] <= rem_bits <= 8
    regions = 1 << b["bits1"]
    leaves = regions << b["bits2"]
    mean1, mean2 = n / regions, n / leaves
    # the mean leaf - and a full one - within the LDS budget
    assert mean2 <= b["leaf_cap"] <= leaf_pairs
    assert leaf_pairs * LDS_BYTES_PER_PAIR + LDS_BYTES_BINS <= LDS_BUDGET
    assert mean2 / (1 << b["rem"]) <= tie_pairs
    # room for every packet, and for the spread of uniform keys
    assert b["region_cap"] * regions >= n and b["leaf_cap"] * leaves >= n
    if slack < 0:
        assert b["region_cap"] >= mean1 + 12. * math.sqrt(mean1)
        assert b["leaf_cap"] >= mean2 + 9. * math.sqrt(mean2)
        assert b["region_cap"] <= mean1 + 12. * math.sqrt(mean1) + 10.
        assert b["leaf_cap"] <= mean2 + 9. * math.sqrt(mean2) + 10.
    else:
        assert b["region_cap"] == max(1, math.ceil(mean1 * (1000 + slack)
                                                   / 1000 - 1e-9))
    # capacities x counts fit the buffers, which do not overlap: the order,
    # the regions, the leaves (pairs of words, on even words)
    assert b["region_begin"] >= n and b["region_begin"] % 2 == 0
    assert b["region_words"] == 2 * b["region_cap"] * regions
    assert b["leaf_begin"] >= b["region_begin"] + b["region_words"]
    assert b["leaf_begin"] % 2 == 0
    assert b["total_words"] == b["leaf_begin"] + 2 * b["leaf_cap"] * leaves
    assert b["region_cap"] < 2 ** 31 and b["total_words"] < 2 ** 34


def test_plan_over_all_launch_sizes(planner):
    cases = [(n, key_bits, -1, -1, -1, 0)
             for n in counts() for key_bits in (0, 5, 12, 16, 17, 22, 24, 32)]
    plans, limits = planner(cases)
    taken = 0
    for (n, key_bits, _, _, _, _), b in zip(cases, plans):
        if not b["take"]:
            continue
        taken += 1
        check_taken(n, key_bits, -1, b, limits)
        # its own choice of bits: a mean leaf of 1024 to 2047 pairs, unless
        # the key or the two levels have no more bits to give
        mean2 = n / (1 << (b["bits1"] + b["bits2"]))
        total = b["bits1"] + b["bits2"]
        assert mean2 >= 1024 or n < 2048
        assert mean2 < 2048 or total == 16 or total == key_bits
        assert b["bits1"] - b["bits2"] in (0, 1)
        # the memory DESIGN.md 3 states: a word per packet for the order, two
        # each for the regions and the leaves, and their room - 12 and 9
        # deviations and 8 pairs per bucket (5.5 words per packet at 1e8)
        regions, leaves = 1 << b["bits1"], 1 << total
        assert b["total_words"] <= (
            5 * n + 24 * math.sqrt(n * regions) + 18 * math.sqrt(n * leaves)
            + 18 * (regions + leaves) + 256)
        if n == 100000000 and key_bits == 24:
            assert b["total_words"] <= 5.52 * n
    assert taken > 1000
    # the old path wherever the leaves would be left more than 8 bits
    for (n, key_bits, _, _, _, _), b in zip(cases, plans):
        total = min(16, max(0, int(math.log2(max(n, 1) / 1024.)))
                    if n >= 1024 else 0)
        if key_bits - total > 8:
            assert not b["take"]


def test_plan_of_the_headline_launch(planner):
    plans, _ = planner([(100000000, 24, -1, -1, -1, 1 << 22),
                        (100000000, 24, -1, -1, -1, 100000001),
                        (10000000, 24, -1, -1, -1, 0),
                        ((1 << 20) + 37, 16, 5, 5, -1, 0),
                        ((1 << 20) + 37, 16, -1, -1, -1, 0)])
    b = plans[0]
    assert (b["take"], b["bits1"], b["bits2"], b["rem"]) == (1, 8, 8, 8)
    assert b["region_cap"] == math.ceil(390625 + 12 * 625 + 8)
    assert b["leaf_cap"] == math.ceil(1e8 / 65536 + 9 * math.sqrt(1e8 / 65536)
                                      + 8)
    assert not plans[1]["take"]  # below the size threshold
    assert not plans[2]["take"]  # 13 bits would leave the leaves 11
    for b in plans[3:]:
        assert (b["take"], b["bits1"], b["bits2"], b["rem"]) == (1, 5, 5, 6)


def test_plan_with_forced_bits_and_slack(planner):
    cases = [(n, key_bits, b1, b2, slack, 0)
             for n in (1, 63, 4097, (1 << 20) + 37, 1 << 27)
             for key_bits in (10, 16, 17, 24)
             for b1 in (0, 3, 5, 8) for b2 in (0, 5, 8)
             for slack in (0, 50, 1000)]
    plans, limits = planner(cases)
    taken = 0
    for (n, key_bits, b1, b2, slack, _), b in zip(cases, plans):
        rem = key_bits - b1 - b2
        if rem < 0 or rem > 8:
            assert not b["take"]
        if b["take"]:
            taken += 1
            assert (b["bits1"], b["bits2"]) == (b1, b2)
            check_taken(n, key_bits, slack, b, limits)
    assert taken > 50
