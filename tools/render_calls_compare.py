"""Compares the outputs and the kernel x calls tables of
tools/render_calls.py under two builds of the library (CMI_GPU_LIBRARY), the
one before a change of the renderers' host code and the one after. DIR holds
calls_parent.npz and calls_new.npz from plain runs, and trace_parent/ and
trace_new/ from runs under `rocprofv3 --kernel-trace --stats --output-format
csv -d DIR/trace_... -- python tools/render_calls.py ...`; the result goes to
DIR/compare_calls.json and the exit status is 1 if anything differs
(profiles/render_driver/).

    python tools/render_calls_compare.py DIR
"""
import csv
import glob
import json
import os
import sys

import numpy as np

OUT = sys.argv[1]


def table(root):
    files = glob.glob(os.path.join(root, "**", "*kernel_stats.csv"),
                      recursive=True)
    assert files, "no kernel_stats.csv under " + root
    calls = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            calls[r["Name"]] = calls.get(r["Name"], 0) + int(r["Calls"])
    return calls


a = np.load(os.path.join(OUT, "calls_parent.npz"))
b = np.load(os.path.join(OUT, "calls_new.npz"))
result = {"bits": {}, "launches": {}}
assert sorted(a.files) == sorted(b.files)
for name in a.files:
    result["bits"][name] = {
        "equal": bool(np.array_equal(a[name], b[name], equal_nan=True)),
        "shape": list(a[name].shape),
        "nonzero": int(np.count_nonzero(a[name]))}
ta, tb = table(os.path.join(OUT, "trace_parent")), table(
    os.path.join(OUT, "trace_new"))
result["launches"] = {"equal": ta == tb, "kernels": len(ta),
                      "calls": sum(ta.values()), "parent": ta, "new": tb}
json.dump(result, open(os.path.join(OUT, "compare_calls.json"), "w"), indent=1)
for name, r in result["bits"].items():
    print("%-36s equal %s %s nonzero %d" % (name, r["equal"], r["shape"],
                                            r["nonzero"]))
print("launch tables equal:", ta == tb, "kernels", len(ta), "calls",
      sum(ta.values()))
for kname in sorted(set(ta) | set(tb)):
    if ta.get(kname) != tb.get(kname):
        print("  differs:", kname, ta.get(kname), tb.get(kname))
ok = ta == tb and all(r["equal"] for r in result["bits"].values())
print("COMPARE_OK" if ok else "COMPARE_DIFFERS")
sys.exit(0 if ok else 1)
