"""Compares the outputs and the kernel x calls tables of
tools/render_calls.py (or tools/scatter_calls.py) under two builds of the
library (CMI_GPU_LIBRARY), the one before a change of the host code and the
one after. DIR holds calls_parent.npz and calls_new.npz from plain runs, and
trace_parent/ and trace_new/ from runs under `rocprofv3 --kernel-trace --stats
--output-format csv -d DIR/trace_... -- python tools/render_calls.py ...`; the
result goes to DIR/compare_calls.json and the exit status is 1 if anything
differs (profiles/render_driver/, profiles/scatter_driver/).

    python tools/render_calls_compare.py DIR [--atomics NAME,NAME,...]

Every output must be np.array_equal, but for those whose last name component
(after the last "/") is listed with --atomics: sums of fp64 atomics in an
order the hardware chooses, held to the rule of the tests' test_additive for
exactly that, rtol 1e-12 and atol 1e-14 of the largest value of the output
(of the images of the same run for an output named cubes).
DIR then also holds calls_parent2.npz, a second plain run of the parent, and
the worst difference of parent against parent is reported next to that of new
against parent, both in units of the tolerance.
"""
import csv
import glob
import json
import os
import sys

import numpy as np

OUT = sys.argv[1]
ATOMICS = sys.argv[3].split(",") if sys.argv[2:3] == ["--atomics"] else []


def table(root):
    files = glob.glob(os.path.join(root, "**", "*kernel_stats.csv"),
                      recursive=True)
    assert files, "no kernel_stats.csv under " + root
    calls = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            calls[r["Name"]] = calls.get(r["Name"], 0) + int(r["Calls"])
    return calls


def excess(got, ref, largest):
    """the worst |got - ref| in units of rtol 1e-12, atol 1e-14 of the
    largest"""
    tol = 1e-12 * np.abs(ref) + 1e-14 * largest
    d = np.abs(got - ref)
    return float(np.where(d > 0., d / np.maximum(tol, 1e-300), 0.).max())


a = np.load(os.path.join(OUT, "calls_parent.npz"))
b = np.load(os.path.join(OUT, "calls_new.npz"))
a2 = np.load(os.path.join(OUT, "calls_parent2.npz")) if ATOMICS else None
result = {"bits": {}, "launches": {}}
assert sorted(a.files) == sorted(b.files)
ok = True
for name in a.files:
    r = {"shape": list(a[name].shape),
         "nonzero": int(np.count_nonzero(a[name]))}
    if name.split("/")[-1] in ATOMICS:
        # a cube is held to the largest I of the images of its run, as the
        # tests hold it
        prefix = name.rsplit("/", 1)[0]
        scale = [m for m in (prefix + "/cube_images", prefix + "/images")
                 if name.endswith("/cubes") and m in a.files] + [name]
        largest = float(np.abs(a[scale[0]]).max())
        r["parent_against_parent"] = excess(a2[name], a[name], largest)
        r["new_against_parent"] = excess(b[name], a[name], largest)
        r["equal"] = r["parent_against_parent"] <= 1. and \
            r["new_against_parent"] <= 1.
    else:
        r["equal"] = bool(np.array_equal(a[name], b[name], equal_nan=True))
    ok = ok and r["equal"]
    result["bits"][name] = r
ta, tb = table(os.path.join(OUT, "trace_parent")), table(
    os.path.join(OUT, "trace_new"))
result["launches"] = {"equal": ta == tb, "kernels": len(ta),
                      "calls": sum(ta.values()), "parent": ta, "new": tb}
if ATOMICS:
    result["worst_in_units_of_the_tolerance"] = {
        k: max(r[k] for r in result["bits"].values() if k in r)
        for k in ("parent_against_parent", "new_against_parent")}
    print(result["worst_in_units_of_the_tolerance"])
json.dump(result, open(os.path.join(OUT, "compare_calls.json"), "w"), indent=1)
for name, r in result["bits"].items():
    print("%-44s %s %s nonzero %d %s" % (
        name, "equal" if "new_against_parent" not in r else "within",
        r["equal"], r["nonzero"],
        "" if "new_against_parent" not in r else "pp %.3g np %.3g" % (
            r["parent_against_parent"], r["new_against_parent"])))
print("launch tables equal:", ta == tb, "kernels", len(ta), "calls",
      sum(ta.values()))
for kname in sorted(set(ta) | set(tb)):
    if ta.get(kname) != tb.get(kname):
        print("  differs:", kname, ta.get(kname), tb.get(kname))
ok = ok and ta == tb
print("COMPARE_OK" if ok else "COMPARE_DIFFERS")
sys.exit(0 if ok else 1)
