#!/usr/bin/env python3
"""After `make -C cmacionize_amd/csrc asm`: what the padded first-generation
kernels hold OUTSIDE their march loop, the general builds next to the bundle
builds (shoot_bundle_kernel, DESIGN_LOG.md 21) and the point build of those
(DESIGN_LOG.md 22).

The march loop is found as tools/march_common_path.py finds it; the outer loop
is the largest loop around it (refill, flush point, end of flights). Per
kernel the tool prints the resources the code object records - VGPRs, SGPR
and VGPR spills, scratch bytes per lane - the common path of the march loop,
and of the outer loop without the march loop: instructions, vector
instructions, lane moves (v_readlane / v_writelane: SGPR spill traffic) and
scratch loads / stores. These are lines of the listing, not executed
instructions: how many of them a bundle runs is for the counters to say.

    python tools/bundle_outer_loop.py [engine.s]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import march_common_path as mcp  # noqa: E402

GENERAL = re.compile(
    r"^(_Z12shoot_kernelILb0ELb0ELb0ELb0ELb1ELb0ELb1ELb[01]ELb0EEv9ShootArgs):")
# (<UNIFORM>, and <true, true>: the point build, DESIGN_LOG.md 22)
BUNDLE = re.compile(
    r"^(_Z19shoot_bundle_kernelILb[01](?:ELb[01])?EEv9ShootArgs"
    r"(?:PK12PointEmitDev)?):")


def kernel_bodies(text):
    """{symbol: lines} of the general and the bundle builds (small blocks, no
    heating term)"""
    out = {}
    for i, l in enumerate(text):
        m = GENERAL.match(l) or BUNDLE.match(l)
        if not m:
            continue
        e = next(j for j in range(i, len(text)) if "s_endpgm" in text[j])
        out[m.group(1)] = text[i:e]
    return out


def resources(text, symbol):
    """the code object's record of a kernel: a dict of its integer fields"""
    name = re.compile(r"\s*\.name:\s+" + re.escape(symbol) + r"\s*$")
    at = next(i for i, l in enumerate(text) if name.match(l))
    lo = at
    while not text[lo].startswith("  - "):
        lo -= 1
    hi = at + 1
    while hi < len(text) and not text[hi].startswith(("  - ", "amdhsa")):
        hi += 1
    out = {}
    for l in text[lo:hi]:
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\d+)\s*$", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def outer_loop(body):
    """(header, last back branch) of the largest loop around the march loop:
    the kernel's loop over rounds"""
    inner = mcp.march_loop(body)
    if inner is None:
        return None, None
    h, e = inner
    loops = []
    for i, l in enumerate(body):
        m = mcp.LABEL.match(l)
        if not m or i >= h:
            continue
        back = [j for j in range(e + 1, len(body))
                if re.search(r"s_c?branch\w*\s+" + re.escape(m.group(1)) +
                             r"\b", body[j])]
        if back:
            loops.append((back[-1] - i, i, back[-1]))
    if not loops:
        return inner, None
    _, oh, oe = max(loops)
    return inner, (oh, oe)


def outer_counts(body):
    inner, outer = outer_loop(body)
    if inner is None or outer is None:
        return None
    (h, e), (oh, oe) = inner, outer
    lines = [t for i, t in mcp.instructions(body[oh:oe + 1])
             if not h <= oh + i <= e]
    return {
        "instructions": len(lines),
        "vector": sum(t.startswith("v_") for t in lines),
        "lane_moves": sum(t.startswith(("v_readlane", "v_writelane"))
                          for t in lines),
        "scratch_loads": sum(t.startswith("scratch_load") for t in lines),
        "scratch_stores": sum(t.startswith("scratch_store") for t in lines),
    }


def report(text):
    """{symbol: dict(resources=, common=, outer=)}"""
    out = {}
    for symbol, body in kernel_bodies(text).items():
        path = mcp.common_path(body)
        out[symbol] = dict(resources=resources(text, symbol),
                           common=mcp.counts(path) if path else None,
                           outer=outer_counts(body), path=path)
    return out


def main(argv):
    path = argv[0] if argv else "cmacionize_amd/csrc/engine.s"
    text = open(path).read().split("\n")
    print("%-62s %5s %6s %6s %8s | %6s %6s | %6s %6s %6s %5s %5s" % (
        "kernel", "vgpr", "s-spl", "v-spl", "scratchB", "vector", "scalar",
        "outer", "vector", "lanemv", "ld", "st"))
    for symbol, r in report(text).items():
        res, c, o = r["resources"], r["common"], r["outer"]
        print("%-62s %5d %6d %6d %8d | %6d %6d | %6d %6d %6d %5d %5d" % (
            symbol, res.get("vgpr_count", -1), res.get("sgpr_spill_count", -1),
            res.get("vgpr_spill_count", -1),
            res.get("private_segment_fixed_size", -1),
            c["vector"] if c else -1, c["scalar"] if c else -1,
            o["instructions"] if o else -1, o["vector"] if o else -1,
            o["lane_moves"] if o else -1, o["scratch_loads"] if o else -1,
            o["scratch_stores"] if o else -1))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
