"""Rate of the H I cubes: the 21-cm line of a lexingtonHII40 state at 256^3
cells (warmed up on the device, tools/converged_state.py) with a radial
expansion v = v0 r / r0 about the centre, a spin temperature of 100 K, the
free-free continuum of the ionized gas and a 2.725 K background, in 64
velocity channels: as 1024^2 pixel cubes for the views theta = 0 and theta =
60 deg, phi = 30 deg, and as the 2048 x 1024 sky map cube of an observer at a
quarter of the box's diagonal.

Per case and per variant of the march kernels (the tuning keys
absorbing_cube_channel_block = 4, 8 and absorbing_cube_expm1_call = 0, 1):
milliseconds of the whole synchronous call (the records, the march per block
of channels, the copy to the host; one warm-up, then --repeats calls: median,
min, max) and the device time of its march launches over the same calls,
median, min and max (the tuning key timing, cmi_gpu_get_kernel_timing). Once
per case the CPU restatement (tests/support/absorbing_cube_reference.c,
OpenMP over OMP_NUM_THREADS threads) on the same machine, fed with the
device's coefficients, and the largest difference to it in units of the tests'
bound. One JSON line per case and variant on stdout and appended to --out.

    python tools/hi_cube_rate.py --out profiles/absorbing_cubes/rate.jsonl
    python tools/hi_cube_rate.py --ncell 64 --pixels 256 --no-cpu
    python tools/hi_cube_rate.py --table profiles/absorbing_cubes/rate.jsonl
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

import absorbing_cube_lib as A  # noqa: E402
import line_image_lib as L  # noqa: E402

VIEWS = [(0., 0.), (np.radians(60.), np.radians(30.))]
VARIANTS = [(4, 1), (4, 0), (8, 1), (8, 0)]
V0 = 20.e3      # m s^-1 at the box's half side
VMIN, VMAX = -60.e3, 60.e3
T_SPIN, T_BACKGROUND = 100., 2.725


def table(path):
    print("| case | CB | expm1 | call ms (min .. max) | march ms (min .. max) "
          "| rays | CPU ms | CPU / call | difference / bound |")
    print("|---|---|---|---|---|---|---|---|---|")
    for line in open(path):
        r = json.loads(line)
        print("| %s | %d | %s | %.0f (%.0f .. %.0f) | %.2f (%.2f .. %.2f) | "
              "%.3g | %s | %s | %s |"
              % (r["case"], r["cb"], "call" if r["expm1_call"] else "inline",
                 r["call_ms_median"], r["call_ms_min"], r["call_ms_max"],
                 r["march_ms"], r["march_ms_min"], r["march_ms_max"],
                 r["rays"],
                 "%.0f" % r["cpu_ms"] if "cpu_ms" in r else "-",
                 "%.1f" % r["speedup"] if "speedup" in r else "-",
                 "%.2g" % r["difference_over_bound"]
                 if "difference_over_bound" in r else "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-sky", action="store_true")
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
    n, nchan = args.pixels, args.channels
    dv = (VMAX - VMIN) / nchan
    # v = V0 r / r0 about the centre of the box, r0 its half side
    centre = box.anchor + 0.5 * box.sides
    axes = [box.anchor[a] + (np.arange(args.ncell) + 0.5) * box.cellside[a] -
            centre[a] for a in range(3)]
    r = np.stack(np.meshgrid(*axes, indexing="ij")).reshape(3, -1)
    vel = V0 * r / (0.5 * box.sides[:, None])
    del r
    eng.set_cell_velocities(vel)
    hi = dict(spin_temperature=T_SPIN, background_temperature=T_BACKGROUND)
    bg = A.host_planck(T_BACKGROUND)
    origin = box.anchor + 0.25 * box.sides
    cases = []
    for theta, phi in VIEWS:
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        cases.append((
            "image %g, %g" % (np.degrees(theta), np.degrees(phi)), n * n,
            lambda theta=theta, phi=phi, anchor=anchor, sides=sides:
            eng.render_hi_cube(theta, phi, n, n, anchor, sides, nchan, VMIN,
                               VMAX, **hi),
            lambda q, theta=theta, phi=phi, anchor=anchor, sides=sides:
            A.cube(box, q["a"], q["sl"], q["b"], theta, phi, n, n, anchor,
                   sides, nchan, VMIN, VMAX, velocity=vel, kc=q["kc"],
                   sc=q["sc"], background=bg), False))
    if not args.no_sky:
        d, _ = E.sky_map_directions(2 * n, n)
        cases.append((
            "sky map %d x %d" % (2 * n, n), 2 * n * n,
            lambda: eng.render_hi_sky_map_cube(origin, 2 * n, n, nchan, VMIN,
                                               VMAX, **hi),
            lambda q: A.sky_cube(box, q["a"], q["sl"], q["b"], origin, d,
                                 nchan, VMIN, VMAX, velocity=vel, kc=q["kc"],
                                 sc=q["sc"],
                                 background=bg).reshape(nchan, 2 * n, n),
            True))
    q = None
    if not args.no_cpu:
        q = eng.hi_coefficients(spin_temperature=T_SPIN)
        depth = A.line_depth(box, q["a"], dv)
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a")
    eng.set_tuning(timing=1)
    for name, rays, call, reference, point in cases:
        ref = cpu_ms = None
        if q is not None:
            t0 = time.perf_counter()
            ref = reference(q)
            cpu_ms = 1e3 * (time.perf_counter() - t0)
            steps = A.longest_ray
        for cb, expm1_call in VARIANTS:
            eng.set_tuning(absorbing_cube_channel_block=cb,
                           absorbing_cube_expm1_call=expm1_call)
            got = call()  # warm-up
            ms, march = [], []
            for _ in range(args.repeats):
                eng.get_timing(reset=True)
                t0 = time.perf_counter()
                got = call()
                ms.append(1e3 * (time.perf_counter() - t0))
                march.append(eng.get_timing(reset=True)["kernel_ms"])
            row = {"case": name, "ncell": args.ncell, "rays": rays,
                   "channels": nchan, "cb": cb, "expm1_call": expm1_call,
                   "call_ms_median": float(np.median(ms)),
                   "call_ms_min": min(ms), "call_ms_max": max(ms),
                   "march_ms": float(np.median(march)),
                   "march_ms_min": min(march), "march_ms_max": max(march),
                   "repeats": args.repeats}
            if ref is not None:
                bound = A.march_bound(steps, depth, q["sl"], q["sc"], bg,
                                      point=point)
                row.update({
                    "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                    "cpu_ms": cpu_ms, "longest_ray": int(steps),
                    "speedup": cpu_ms / row["call_ms_median"],
                    "difference_over_bound":
                        float(np.abs(got - ref).max() / bound)})
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del got
    eng.close()
    del backend
    return 0


if __name__ == "__main__":
    sys.exit(main())
