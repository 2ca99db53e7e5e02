"""Rate of the emission-line images: 4 lines (HAlpha, HBeta, OIII_5007,
NII_6584) at 1024^2 pixels of a lexingtonHII40 state at 256^3 cells (warmed
up on the device, tools/converged_state.py), for the views theta = 0 and
theta = 60 deg, phi = 30 deg, without and with dust, at supersampling 1 and 2.

Per case: milliseconds of the whole synchronous call (records, march, the
images' copy to the host; one warm-up, then --repeats calls: median, min,
max), cell crossings per second, and the same case on the CPU restatement
(tests/support/line_image_reference.c, OpenMP over OMP_NUM_THREADS threads;
it also counts the crossings). The GPU has to beat the restatement in every
case: gpu_beats_cpu says so per case and the exit status is 1 if one does
not. One JSON line per case on stdout and appended to --out.

Bytes per crossing against the record size need a counter run of their own:
--once renders the first case once, to be run under
`rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR`; a later run with
--counters DIR divides what the march kernel fetched there (KiB per
dispatch, summed) by the crossings of that case and adds
fetched_bytes_per_crossing to its line. --table FILE prints the lines of a
jsonl file as the table of DESIGN.md 4.7 and does nothing else.

    python tools/line_image_rate.py --out profiles/line_images/rate.jsonl
    python tools/line_image_rate.py --ncell 64 --pixels 256 --no-cpu
    python tools/line_image_rate.py --table profiles/line_images/rate.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import line_image_lib as L  # noqa: E402

LINES = ["HAlpha", "HBeta", "OIII_5007", "NII_6584"]
VIEWS = [(0., 0.), (np.radians(60.), np.radians(30.))]
SIGMA = 2.e-27  # m^2 per H: optical depth ~6 through 10 pc of 1e8 m^-3


def march_fetch_bytes(root):
    """bytes line_image_march_kernel fetched in the counter run under root"""
    import csv
    import glob
    kib = 0.
    files = glob.glob(os.path.join(root, "**", "*counter_collection.csv"),
                      recursive=True)
    if not files:
        raise SystemExit("no counter_collection.csv under " + root)
    for f in files:
        for r in csv.DictReader(open(f)):
            if ("line_image_march_kernel" in r["Kernel_Name"] and
                    r["Counter_Name"] == "FETCH_SIZE"):
                kib += float(r["Counter_Value"])
    return 1024. * kib


def table(path):
    print("| view | dust | s | GPU ms (min .. max) | crossings | GPU /s | "
          "CPU ms | GPU / CPU | B / crossing |")
    print("|---|---|---|---|---|---|---|---|---|")
    for line in open(path):
        r = json.loads(line)
        fetched = r.get("fetched_bytes_per_crossing")
        print("| %g, %g | %s | %d | %.1f (%.1f .. %.1f) | %.3g | %.3g | %s | "
              "%s | %s |" % (
                  r["theta_deg"], r["phi_deg"], "yes" if r["dust"] else "no",
                  r["supersample"], r["gpu_ms_median"], r["gpu_ms_min"],
                  r["gpu_ms_max"], r.get("crossings", float("nan")),
                  r.get("gpu_crossings_per_s", float("nan")),
                  "%.0f" % r["cpu_ms"] if "cpu_ms" in r else "-",
                  "%.1f" % r["speedup"] if "speedup" in r else "-",
                  "%.1f of %d" % (fetched, r["record_bytes"]) if fetched
                  else "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None)
    ap.add_argument("--counters", default=None)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--supersample", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--once", action="store_true",
                    help="one case, one call (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.table:
        return table(args.table)
    fetched = march_fetch_bytes(args.counters) if args.counters else None
    slower = 0

    import converged_state
    from cmacionize_amd import STROMGREN as S
    t0 = time.perf_counter()
    backend = converged_state.lexington_state(args.ncell, args.iterations,
                                              int(args.packets))
    eng = backend.engine
    eng.synchronize()
    print("state: %d^3 after %d iterations of %g packets, %.1f s" %
          (args.ncell, args.iterations, args.packets,
           time.perf_counter() - t0), file=sys.stderr)
    box = L.Box(S["anchor"], S["sides"], (args.ncell,) * 3)
    n = args.pixels
    record_bytes = 8 * ((len(LINES) + 2) & ~1)
    j = density = None
    if not args.no_cpu and not args.once:
        em = eng.compute_emissivities(LINES)
        j = np.array([em[name] for name in LINES])
        from cmacionize_amd import engine as E
        density = eng.download_field(E.FIELD_NUMBER_DENSITY)
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a")
    for theta, phi in VIEWS:
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        for sigma in (0., SIGMA):
            for s in args.supersample:
                call = lambda: eng.render_line_images(
                    LINES, theta, phi, n, n, anchor, sides, s, sigma)
                images = call()  # warm-up
                if args.once:
                    return
                ms = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    images = call()
                    ms.append(1e3 * (time.perf_counter() - t0))
                row = {"ncell": args.ncell, "pixels": n, "lines": len(LINES),
                       "theta_deg": float(np.degrees(theta)),
                       "phi_deg": float(np.degrees(phi)), "dust": sigma > 0.,
                       "supersample": s, "record_bytes": record_bytes,
                       "gpu_ms_median": float(np.median(ms)),
                       "gpu_ms_min": min(ms), "gpu_ms_max": max(ms),
                       "repeats": args.repeats}
                if j is not None:
                    t0 = time.perf_counter()
                    ref = L.render(box, j, theta, phi, n, n, anchor, sides, s,
                                   extinction=density * sigma if sigma
                                   else None)
                    cpu_ms = 1e3 * (time.perf_counter() - t0)
                    crossings = L.last_crossings
                    got = np.array([images[name] for name in LINES])
                    lit = ref > 0.
                    row.update({
                        "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                        "cpu_ms": cpu_ms, "crossings": crossings,
                        "gpu_crossings_per_s":
                            crossings / (1e-3 * row["gpu_ms_median"]),
                        "cpu_crossings_per_s": crossings / (1e-3 * cpu_ms),
                        "speedup": cpu_ms / row["gpu_ms_median"],
                        "gpu_beats_cpu": row["gpu_ms_max"] < cpu_ms,
                        "worst_relative_difference": float(
                            (np.abs(got - ref)[lit] / ref[lit]).max())})
                    slower += not row["gpu_beats_cpu"]
                    if fetched is not None:
                        # the counter run rendered the first case
                        row["fetched_bytes_per_crossing"] = fetched / crossings
                        fetched = None
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    eng.close()
    del backend
    if slower:
        print("%d cases in which the GPU does not beat the restatement" %
              slower, file=sys.stderr)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
