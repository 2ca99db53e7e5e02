#!/usr/bin/env python3
"""After `make -C cmacionize_amd/csrc asm`: the march loop of every
line_image_march_kernel<ND> (ND = doubles per record: 2, 4, 6, 8) in
engine.s - the loop that holds the record's loads - with its size and what
must not be in it: scratch (spill) accesses and atomics.

    python tools/line_image_loop.py [cmacionize_amd/csrc/engine.s]
exit code 1 if a kernel is missing or its loop has either."""
import re
import sys

KERNEL = re.compile(r"^_Z23line_image_march_kernelILi(\d+)EEv13LineMarchArgs:")


def loops_of(body):
    """(label line, line of the last branch back to it) of every loop"""
    found = []
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if not m:
            continue
        back = [j for j in range(i + 1, len(body))
                if re.search(r"s_c?branch\w*\s+" + re.escape(m.group(1)) +
                             r"\b", body[j])]
        if back:
            found.append((i, back[-1]))
    return found


def scan(text):
    """{ND: counts of the march loop} from the listing's lines"""
    out = {}
    for s, line in enumerate(text):
        m = KERNEL.match(line)
        if not m:
            continue
        e = next(i for i in range(s, len(text)) if "s_endpgm" in text[i])
        body = text[s:e]
        loads = [i for i, l in enumerate(body) if "global_load" in l]
        around = [(e2 - h2, h2, e2) for h2, e2 in loops_of(body)
                  if any(h2 < i < e2 for i in loads)]
        if not around:
            continue
        _, h, end = max(around)
        loop = [l.strip() for l in body[h:end + 1]]
        count = lambda p: sum(1 for l in loop if l.startswith(p))
        out[int(m.group(1))] = {
            "lines": len(loop), "valu": count("v_"), "salu": count("s_"),
            "f64": sum(1 for l in loop if re.match(r"v_\w+_f64", l)),
            "loads": count("global_load"),
            "scratch": sum(1 for l in loop if "scratch_" in l),
            "atomic": sum(1 for l in loop if "atomic" in l),
            "calls": count("s_swappc"),
        }
    return out


def report(text):
    found = scan(text)
    print("%-28s %6s %6s %6s %6s %6s %8s %7s" % (
        "line_image_march_kernel<ND>", "lines", "valu", "f64", "salu",
        "loads", "scratch", "atomic"))
    bad = 0
    for nd in (2, 4, 6, 8):
        c = found.get(nd)
        if c is None:
            print("<%d>: not found" % nd)
            bad = 1
            continue
        print("%-28s %6d %6d %6d %6d %6d %8d %7d" % (
            "<%d>" % nd, c["lines"], c["valu"], c["f64"], c["salu"],
            c["loads"], c["scratch"], c["atomic"]))
        if c["scratch"] or c["atomic"] or c["calls"]:
            bad = 1
    return bad


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else "cmacionize_amd/csrc/engine.s"
    sys.exit(report(open(path).read().split("\n")))
