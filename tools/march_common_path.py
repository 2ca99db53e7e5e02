#!/usr/bin/env python3
"""After `make -C cmacionize_amd/csrc asm`: the COMMON PATH of the padded
hydrogen-only march loop, instruction by instruction.

tools/check_hot_loops.py sizes the whole march loop, probe chain and end of
flight included. What a wave trip executes nearly always is much shorter: every
lane finds its table slot at the first probe and no flight ends. That path is

    loop header .. the first exit branch after the first ds_add_f64
    (the "every lane found its slot" test), without the end-of-flight block,
    + the blocks that branch runs through on its way back to the header

and the loop is bound by instruction issue, so its counts of
vector and of scalar lines - nops, waits and branches included - are what the
kernel's time follows.

    python tools/march_common_path.py [engine.s] [-v]
prints one line per hydrogen-only PAD variant <F=0,...,PAD=1>; -v lists the
path. The end-of-flight block is the largest `s_cbranch_execz L` .. `L:` region
that holds the v_rcp_f64 of the path-length correction and not the march's
v_min_f64.
"""
import re
import sys

KERNEL = re.compile(r"^_Z12shoot_kernelI((?:Lb[01]E){6,9})Ev9ShootArgs:")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s*(s_c?branch\w*)\s+(\.LBB\d+_\d+)\b")


def instructions(lines):
    """(index, text) of the lines that are instructions"""
    out = []
    for i, l in enumerate(lines):
        s = l.strip()
        if not s or s.startswith(";") or s.startswith(".") or LABEL.match(l):
            continue
        out.append((i, s.split(";")[0].strip()))
    return out


def march_loop(body):
    """(header, last back branch) of the march loop of a kernel body - the
    same rule as tools/check_hot_loops.py - or None"""
    cas = [i for i, l in enumerate(body) if "ds_cmpst" in l]
    if not cas:
        return None
    loops = []
    for i, l in enumerate(body):
        m = LABEL.match(l)
        if not m:
            continue
        back = [j for j in range(i + 1, len(body))
                if re.search(r"s_c?branch\w*\s+" + re.escape(m.group(1)) +
                             r"\b", body[j])]
        if back:
            loops.append((i, back[-1]))
    around = [(e - h, h, e) for h, e in loops
              if h < cas[0] < e and e - h > 100]
    if not around:
        return None
    _, h, e = min(around)
    return h, e


def end_of_flight(body, lo, hi):
    """(first, last) line of the end-of-flight block inside body[lo:hi], or
    None"""
    labels = {LABEL.match(l).group(1): i for i, l in enumerate(body)
              if LABEL.match(l)}
    best = None
    for i in range(lo, hi):
        m = BRANCH.match(body[i])
        if not m or m.group(1) != "s_cbranch_execz":
            continue
        j = labels.get(m.group(2), -1)
        if not i < j <= hi:
            continue
        region = body[i + 1:j]
        if any("v_rcp_f64" in l for l in region) and \
                not any("v_min_f64" in l for l in region):
            if best is None or j - i > best[1] - best[0]:
                best = (i + 1, j - 1)
    return best


def common_path(body):
    """the instructions of the common path of a kernel body, as a list of
    texts, or None if the kernel has no march loop with a table"""
    loop = march_loop(body)
    if loop is None:
        return None
    h, end = loop
    labels = {LABEL.match(l).group(1): i for i, l in enumerate(body)
              if LABEL.match(l)}
    header = LABEL.match(body[h]).group(1)
    add = next((i for i in range(h, end + 1) if "ds_add_f64" in body[i]), None)
    if add is None:
        return None
    # the first branch after the first ds_add_f64: "all lanes found a slot"
    exit_branch = next(i for i in range(add, end + 1) if BRANCH.match(body[i]))
    skip = end_of_flight(body, h, exit_branch)
    path = [t for i, t in instructions(body[h:exit_branch + 1])
            if skip is None or not skip[0] <= h + i <= skip[1]]
    # the way back to the header (taken conditional branches and fall-through
    # both count: the structurised exit is a chain of them)
    # the way back to the header: s_branch is followed, a conditional branch
    # is taken if it goes to the header and falls through otherwise (it is
    # the loop's exit)
    at = labels[BRANCH.match(body[exit_branch]).group(2)]
    for _ in range(256):
        if at == h or at >= len(body):
            break
        l = body[at]
        s = l.strip()
        if s and not s.startswith(";") and not s.startswith(".") and \
                not LABEL.match(l):
            path.append(s.split(";")[0].strip())
        m = BRANCH.match(l)
        if m and (m.group(1) == "s_branch" or m.group(2) == header):
            at = labels[m.group(2)]
        else:
            at += 1
    return path


def counts(path):
    is_ = lambda p: sum(1 for t in path if t.startswith(p))
    return {
        "vector": is_("v_"),
        "scalar": is_("s_"),
        "nops": is_("s_nop"),
        "waits": is_("s_waitcnt"),
        "branches": sum(1 for t in path if re.match(r"s_c?branch", t)),
        "global": is_("global_"),
        "lds": is_("ds_"),
        "scratch": sum(1 for t in path if "scratch_" in t),
        "readlane": sum(1 for t in path if "v_readlane" in t),
    }


def scan(text):
    """{flags tuple: path} for the hydrogen-only PAD variants of engine.s"""
    out = {}
    starts = [i for i, l in enumerate(text) if KERNEL.match(l)]
    for s in starts:
        flags = tuple(re.findall(r"Lb([01])E", KERNEL.match(text[s]).group(1)))
        if len(flags) < 7 or flags[0] != "0" or flags[6] != "1":
            continue
        e = next(i for i in range(s, len(text)) if "s_endpgm" in text[i])
        path = common_path(text[s:e])
        if path is not None:
            out[flags] = path
    return out


def main(argv):
    verbose = "-v" in argv
    args = [a for a in argv if a != "-v"]
    path = args[0] if args else "cmacionize_amd/csrc/engine.s"
    found = scan(open(path).read().split("\n"))
    print("%-22s %6s %6s %5s %5s %8s %6s %4s %7s %8s" % (
        "variant <F,H,R,X,T,P,PAD,TRK,Q>", "vector", "scalar", "nops",
        "waits", "branches", "global", "lds", "scratch", "readlane"))
    for flags, p in found.items():
        c = counts(p)
        print("%-22s %6d %6d %5d %5d %8d %6d %4d %7d %8d" % (
            "<%s>" % ",".join(flags), c["vector"], c["scalar"], c["nops"],
            c["waits"], c["branches"], c["global"], c["lds"], c["scratch"],
            c["readlane"]))
        if verbose:
            for t in p:
                print("    " + t)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
