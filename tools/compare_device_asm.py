"""Compare the device code of two builds function by function, without a GPU.

Both arguments are assembly files of engine.hip made with the Makefile's flags
(`make -C cmacionize_amd/csrc asm` leaves csrc/engine.s; for the parent commit
the same command in a checkout of it). Labels, directives and comments are
removed and a function's instructions are compared line by line. Prints how
many of the first file's functions are the same in the second, which differ or
are gone, and for every function the second file adds its number of
instructions and of scratch / buffer memory instructions (spill code and
stack traffic).

    python tools/compare_device_asm.py parent/engine.s csrc/engine.s

A function that only changed its name - a template parameter it gained, whose
new instantiations are reported as new functions - is still the parent's if
its instructions are: `--rename PARENT_SYMBOL=NEW_SYMBOL` (any number of
them) renames the symbol in the parent's listing, in the calls to it too,
before the comparison.
"""
import re
import sys


def functions(path):
    out = {}
    name = None
    for line in open(path):
        m = re.match(r"\s*\.type\s+([^,]+),@function", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip() or re.match(r"^[.\w$]+:\s*$", s) or \
                s.strip().startswith("."):
            continue
        out[name].append(re.sub(r"\.LBB\d+_\d+", ".L", s.strip()))
    return out


def renamed(funcs, pairs):
    """`funcs` with the symbols of `pairs` renamed, longest first (a symbol
    may be the beginning of another)"""
    pairs = sorted(pairs, key=lambda p: -len(p[0]))

    def sub(text):
        for old, new in pairs:
            text = re.sub(r"(?<![\w$])" + re.escape(old) + r"(?![\w$])", new,
                          text)
        return text
    return {sub(k): [sub(s) for s in v] for k, v in funcs.items()}


def main():
    args = sys.argv[1:]
    pairs = []
    while "--rename" in args:
        i = args.index("--rename")
        pairs.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    parent, new = functions(args[0]), functions(args[1])
    if pairs:
        parent = renamed(parent, pairs)
        print("renamed in the parent:", ["%s -> %s" % p for p in pairs])
    same = [k for k in parent if new.get(k) == parent[k]]
    print("%d of %d parent functions identical" % (len(same), len(parent)))
    print("differing:", [k for k in parent if k in new and new[k] != parent[k]])
    print("gone:", [k for k in parent if k not in new])
    dust = [k for k in parent if "dust" in k]
    print("of them with 'dust' in the name: %d, identical: %d" %
          (len(dust), sum(k in same for k in dust)))
    print("new functions {instructions, scratch or buffer memory "
          "instructions}:")
    for k in new:
        if k in parent:
            continue
        mem = sum(1 for s in new[k] if s.startswith(("scratch_", "buffer_")))
        print("  %s {%d, %d}" % (k, len(new[k]), mem))
    return 0


if __name__ == "__main__":
    sys.exit(main())
