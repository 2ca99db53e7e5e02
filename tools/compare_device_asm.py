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


def main():
    parent, new = functions(sys.argv[1]), functions(sys.argv[2])
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
