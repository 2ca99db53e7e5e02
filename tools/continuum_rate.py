"""Rate of the continuum images: free-free emission of a lexingtonHII40 state
at 256^3 cells (warmed up on the device, tools/converged_state.py) at 16
frequencies from 100 MHz to 100 GHz, as 1024^2 pixel images for the views
theta = 0 and theta = 60 deg, phi = 30 deg, and as the 2048 x 1024 sky map of
an observer at a quarter of the box's diagonal.

Per case and per channel block FB = 4, 8, 16 (the tuning key
continuum_channel_block): milliseconds of the whole synchronous call (the
records, the march per block of channels, the copy to the host; one warm-up,
then --repeats calls: median, min, max) and the device time of its march
launches over the same calls, median, min and max (the tuning key timing,
cmi_gpu_get_kernel_timing). Once per case the CPU restatement (tests/support/continuum_reference.c, OpenMP over
OMP_NUM_THREADS threads) on the same machine, fed with the device's
free-free coefficients, and the largest difference to it in units of the
tests' bound. One JSON line per case and FB on stdout and appended to --out.

    python tools/continuum_rate.py --out profiles/continuum/rate.jsonl
    python tools/continuum_rate.py --ncell 64 --pixels 256 --no-cpu
    python tools/continuum_rate.py --table profiles/continuum/rate.jsonl
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

import continuum_lib as K  # noqa: E402
import line_image_lib as L  # noqa: E402

VIEWS = [(0., 0.), (np.radians(60.), np.radians(30.))]
BLOCKS = (4, 8, 16)


def table(path):
    print("| case | FB | call ms (min .. max) | march ms (min .. max) | rays "
          "| CPU ms | CPU / call | difference / bound |")
    print("|---|---|---|---|---|---|---|---|")
    for line in open(path):
        r = json.loads(line)
        print("| %s | %d | %.1f (%.1f .. %.1f) | %.2f (%.2f .. %.2f) | %.3g | "
              "%s | %s | %s |"
              % (r["case"], r["fb"], r["call_ms_median"], r["call_ms_min"],
                 r["call_ms_max"], r["march_ms"],
                 r.get("march_ms_min", r["march_ms"]),
                 r.get("march_ms_max", r["march_ms"]), r["rays"],
                 "%.0f" % r["cpu_ms"] if "cpu_ms" in r else "-",
                 "%.1f" % r["speedup"] if "speedup" in r else "-",
                 "%.2g" % r["difference_over_bound"]
                 if "difference_over_bound" in r else "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--frequencies", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    import converged_state
    from cmacionize_amd import STROMGREN as S
    from cmacionize_amd import engine as E
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
    nu = 10. ** np.linspace(8., 11., args.frequencies)
    bg = E.planck_function(nu, 2.725)
    origin = box.anchor + 0.25 * box.sides
    cases = []
    for theta, phi in VIEWS:
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        cases.append((
            "image %g, %g" % (np.degrees(theta), np.degrees(phi)), n * n,
            lambda theta=theta, phi=phi, anchor=anchor, sides=sides:
            eng.render_continuum_images(nu, theta, phi, n, n, anchor, sides,
                                        background=bg),
            lambda k, s, theta=theta, phi=phi, anchor=anchor, sides=sides:
            K.images(box, k, s, theta, phi, n, n, anchor, sides,
                     background=bg), False))
    d, _ = E.sky_map_directions(2 * n, n)
    cases.append((
        "sky map %d x %d" % (2 * n, n), 2 * n * n,
        lambda: eng.render_continuum_sky_map(nu, origin, 2 * n, n,
                                             background=bg),
        lambda k, s: K.sky(box, k, s, origin, d,
                           background=bg).reshape(len(nu), 2 * n, n), True))
    kappa = source = None
    if not args.no_cpu:
        kappa, source = eng.free_free_coefficients(nu)
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a")
    eng.set_tuning(timing=1)
    for name, rays, call, reference, point in cases:
        ref = cpu_ms = None
        if kappa is not None:
            t0 = time.perf_counter()
            ref = reference(kappa, source)
            cpu_ms = 1e3 * (time.perf_counter() - t0)
            steps = K.longest_ray
        for fb in BLOCKS:
            eng.set_tuning(continuum_channel_block=fb)
            got = call()  # warm-up
            ms, march = [], []
            for _ in range(args.repeats):
                eng.get_timing(reset=True)
                t0 = time.perf_counter()
                got = call()
                ms.append(1e3 * (time.perf_counter() - t0))
                march.append(eng.get_timing(reset=True)["kernel_ms"])
            row = {"case": name, "ncell": args.ncell, "rays": rays,
                   "frequencies": len(nu), "fb": fb,
                   "call_ms_median": float(np.median(ms)),
                   "call_ms_min": min(ms), "call_ms_max": max(ms),
                   "march_ms": float(np.median(march)),
                   "march_ms_min": min(march), "march_ms_max": max(march),
                   "repeats": args.repeats}
            if ref is not None:
                worst = max(
                    np.abs(got[f] - ref[f]).max() /
                    K.march_bound(steps, source[f], bg[f:f + 1], point=point)
                    for f in range(len(nu)))
                row.update({
                    "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                    "cpu_ms": cpu_ms, "longest_ray": int(steps),
                    "speedup": cpu_ms / row["call_ms_median"],
                    "difference_over_bound": float(worst)})
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
