"""Rate of the sky maps: 4 lines (HAlpha, HBeta, OIII_5007, NII_6584) as a
2048 x 1024 full-sky map of a lexingtonHII40 state at 256^3 cells (warmed up
on the device, tools/converged_state.py), for an observer at the box centre
and near a corner, without and with dust, with the rays in 8 x 8 tiles of the
map (cmi_gpu_render_line_sky_map) and in plain pixel order
(cmi_gpu_render_line_sky on sky_map_directions' rays).

Per case: milliseconds of the whole synchronous call (records, directions up,
march, results down, and for the map call the directions and the reordering
on the host; one warm-up, then --repeats calls: median, min, max), cell
crossings per second, and the same rays on the CPU restatement
(tests/support/sky_image_reference.c, OpenMP over OMP_NUM_THREADS threads; it
also counts the crossings). One JSON line per case on stdout and appended to
--out. --once renders the first case once, to be run under `rocprofv3
--kernel-trace --stats` for the march's own share of a call. --table FILE
prints the lines of a jsonl file as the table of DESIGN.md 4.9 and does
nothing else.

    python tools/sky_map_rate.py --out profiles/sky_maps/rate.jsonl
    python tools/sky_map_rate.py --ncell 64 --nlon 256 --nlat 128 --no-cpu
    python tools/sky_map_rate.py --table profiles/sky_maps/rate.jsonl
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

import sky_image_lib as S  # noqa: E402

LINES = ["HAlpha", "HBeta", "OIII_5007", "NII_6584"]
SIGMA = 2.e-27  # m^2 per H: optical depth ~6 through 10 pc of 1e8 m^-3
# the observer, as fractions of the box sides from the anchor
OBSERVERS = {"centre": (0.5, 0.5, 0.5), "corner": (0.05, 0.08, 0.03)}


def table(path):
    print("| observer | dust | ray order | GPU ms (min .. max) | crossings | "
          "GPU /s | CPU ms | GPU / CPU |")
    print("|---|---|---|---|---|---|---|---|")
    for line in open(path):
        r = json.loads(line)
        print("| %s | %s | %s | %.1f (%.1f .. %.1f) | %.3g | %.3g | %s | %s |"
              % (r["observer"], "yes" if r["dust"] else "no", r["order"],
                 r["gpu_ms_median"], r["gpu_ms_min"], r["gpu_ms_max"],
                 r.get("crossings", float("nan")),
                 r.get("gpu_crossings_per_s", float("nan")),
                 "%.0f" % r["cpu_ms"] if "cpu_ms" in r else "-",
                 "%.1f" % r["speedup"] if "speedup" in r else "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--nlon", type=int, default=2048)
    ap.add_argument("--nlat", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--once", action="store_true",
                    help="one case, one call (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    import converged_state
    from cmacionize_amd import STROMGREN as ST
    from cmacionize_amd import engine as E
    t0 = time.perf_counter()
    backend = converged_state.lexington_state(args.ncell, args.iterations,
                                              int(args.packets))
    eng = backend.engine
    eng.synchronize()
    print("state: %d^3 after %d iterations of %g packets, %.1f s" %
          (args.ncell, args.iterations, args.packets,
           time.perf_counter() - t0), file=sys.stderr)
    box = S.Box(ST["anchor"], ST["sides"], (args.ncell,) * 3)
    nlon, nlat = args.nlon, args.nlat
    directions, _ = E.sky_map_directions(nlon, nlat)
    j = density = None
    if not args.no_cpu and not args.once:
        em = eng.compute_emissivities(LINES)
        j = np.array([em[name] for name in LINES])
        density = eng.download_field(E.FIELD_NUMBER_DENSITY)
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a")
    for observer, fraction in OBSERVERS.items():
        origin = box.anchor + box.sides * np.array(fraction)
        for sigma in (0., SIGMA):
            ref = cpu_ms = crossings = None
            if j is not None:
                t0 = time.perf_counter()
                ref = S.render(box, j, origin, directions,
                               extinction=density * sigma if sigma else None)
                cpu_ms = 1e3 * (time.perf_counter() - t0)
                crossings = S.last_crossings
            calls = {
                "tiles": lambda: eng.render_line_sky_map(
                    LINES, origin, nlon, nlat, dust_cross_section=sigma),
                "pixels": lambda: eng.render_line_sky(
                    LINES, origin, directions, sigma)}
            # the two orders alternate, so that whatever else the machine
            # does falls on both
            ms = {order: [] for order in calls}
            got = {order: call() for order, call in calls.items()}  # warm-up
            if args.once:
                return 0
            for _ in range(args.repeats):
                for order, call in calls.items():
                    t0 = time.perf_counter()
                    got[order] = call()
                    ms[order].append(1e3 * (time.perf_counter() - t0))
            for order in calls:
                row = {"ncell": args.ncell, "nlon": nlon, "nlat": nlat,
                       "lines": len(LINES), "observer": observer,
                       "dust": sigma > 0., "order": order,
                       "gpu_ms_median": float(np.median(ms[order])),
                       "gpu_ms_min": min(ms[order]),
                       "gpu_ms_max": max(ms[order]), "repeats": args.repeats}
                if ref is not None:
                    values = np.array([got[order][name].reshape(-1)
                                       for name in LINES])
                    lit = ref > 0.
                    row.update({
                        "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                        "cpu_ms": cpu_ms, "crossings": crossings,
                        "gpu_crossings_per_s":
                            crossings / (1e-3 * row["gpu_ms_median"]),
                        "cpu_crossings_per_s": crossings / (1e-3 * cpu_ms),
                        "speedup": cpu_ms / row["gpu_ms_median"],
                        "worst_relative_difference": float(
                            (np.abs(values - ref)[lit] / ref[lit]).max())})
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    eng.close()
    del backend
    return 0


if __name__ == "__main__":
    sys.exit(main())
