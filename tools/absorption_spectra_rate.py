"""Rate of the absorption spectra: the 14 resonance lines of
ABSORPTION_LINES through a lexingtonHII40 state at 256^3 cells (warmed up on
the device, tools/converged_state.py) with a radial expansion v = v0 r / r0
about the centre and a turbulent dispersion of 2 km/s, along 1024 sightlines -
256 from each of four points outside the box towards random points of it, to
the edge of the box - in 1024 velocity channels over +-200 km/s.

Per variant of the march kernel (the tuning keys absorption_slab_rows = 1, 2,
4, absorption_edge_sharing = 1, 0, and once absorption_skips = 0):
milliseconds of the whole synchronous call of render_absorption_spectra (the
records, the march, the copy to the host; one warm-up, then --repeats calls:
median, min, max) and the device time of its march launch over the same calls
(the tuning key timing). Two baselines on the same machine, each once:

* the CPU restatement (tests/support/absorption_reference.c, OpenMP over
  OMP_NUM_THREADS threads), fed with the same densities and widths formed in
  numpy, and the largest difference to it in units of the tests' bound;
* what a user could do before: render_field_absorbing_sky_cube(a = S n, sl =
  0, b) once per line and origin on the same rays and axis - Gaussian
  profiles only, so the spectra are compared to it with g = 0.

--label names the library the rows come from (a build with
-DCMI_ABSORPTION_WALK_ONLY, loaded through CMI_GPU_LIBRARY, gives the share of
the walk). One JSON line per row on stdout and appended to --out.

    python tools/absorption_spectra_rate.py --out profiles/absorption_spectra/rate.jsonl
    python tools/absorption_spectra_rate.py --ncell 64 --rays 64 --no-cpu
    python tools/absorption_spectra_rate.py --table profiles/absorption_spectra/rate.jsonl
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

import absorption_lib as AB  # noqa: E402
import line_image_lib as L  # noqa: E402

V0 = 20.e3      # m s^-1 at the box's half side
SIGMA_TURB = 2.e3
VMIN, VMAX = -200.e3, 200.e3
VARIANTS = [(1, 1, 1), (2, 1, 1), (4, 1, 1), (1, 0, 1), (2, 0, 1), (4, 0, 1),
            (None, 1, 0)]
BOLTZMANN, ATOMIC_MASS_UNIT = 1.38064852e-23, 1.660539040e-27


def table(path):
    print("| label | case | R | sharing | skips | call ms (min .. max) | "
          "march ms (min .. max) | over the call | difference / bound |")
    print("|---|---|---|---|---|---|---|---|---|")
    for line in open(path):
        r = json.loads(line)
        if "call_ms_median" in r:
            print("| %s | spectra | %d | %s | %s | %.1f (%.1f .. %.1f) | "
                  "%.2f (%.2f .. %.2f) | 1 | - |"
                  % (r["label"], r["rows"], "on" if r["sharing"] else "off",
                     "on" if r["skips"] else "off", r["call_ms_median"],
                     r["call_ms_min"], r["call_ms_max"], r["march_ms"],
                     r["march_ms_min"], r["march_ms_max"]))
        else:
            print("| %s | %s | - | - | - | %.0f | %s | %.1f | %s |"
                  % (r["label"], r["case"], r["ms"],
                     "%.1f" % r["march_ms"] if "march_ms" in r else "-",
                     r["over_the_call"],
                     "%.2g" % r["difference_over_bound"]
                     if "difference_over_bound" in r else "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--label", default="this")
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
    nchan = args.channels
    dv = (VMAX - VMIN) / nchan
    centre = box.anchor + 0.5 * box.sides
    axes = [box.anchor[a] + (np.arange(args.ncell) + 0.5) * box.cellside[a] -
            centre[a] for a in range(3)]
    r = np.stack(np.meshgrid(*axes, indexing="ij")).reshape(3, -1)
    vel = V0 * r / (0.5 * box.sides[:, None])
    del r
    eng.set_cell_velocities(vel)

    # four points outside the box, a quarter of the rays from each, towards
    # random points of the box
    rng = np.random.default_rng(2)
    corners = np.array([(1.6, 0.3, 0.1), (-1.4, -1.2, 0.5), (0.2, 1.7, -1.3),
                        (-0.6, 0.4, 1.9)])
    points = centre + 0.5 * box.sides * corners
    per = args.rays // len(points)
    origins = np.repeat(points, per, axis=0)
    towards = box.anchor + box.sides * rng.uniform(0.05, 0.95,
                                                   (len(origins), 3))
    d = towards - origins
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    lengths = np.full(len(d), np.inf)
    names = list(E.ABSORPTION_LINES)
    ions, weights, Sl, gl, _ = E.absorption_table_lines(names)

    def call(g=gl):
        lines = [(ions[k], weights[k], Sl[k], g[k]) for k in range(len(names))]
        return eng.render_absorption_spectra(lines, origins, d, nchan, VMIN,
                                             VMAX, lengths=lengths,
                                             sigma_turb=SIGMA_TURB)

    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a")

    def emit(row):
        row = dict({"label": args.label, "ncell": args.ncell,
                    "rays": len(d), "lines": len(names), "channels": nchan},
                   **row)
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    eng.set_tuning(timing=1)
    # (the rule of render_driver.h for absorption_slab_rows = 0)
    default_rows = 1 if nchan <= 64 else (2 if nchan <= 128 else
                                          AB.default_rows())
    default = None
    for rows, sharing, skips in VARIANTS:
        eng.set_tuning(absorption_slab_rows=rows or 0,
                       absorption_edge_sharing=sharing,
                       absorption_skips=skips)
        call()  # warm-up
        ms, march = [], []
        for _ in range(args.repeats):
            eng.get_timing(reset=True)
            t0 = time.perf_counter()
            got = call()
            ms.append(1e3 * (time.perf_counter() - t0))
            march.append(eng.get_timing(reset=True)["kernel_ms"])
        rows = rows or default_rows
        emit({"rows": rows, "sharing": sharing, "skips": skips,
              "call_ms_median": float(np.median(ms)), "call_ms_min": min(ms),
              "call_ms_max": max(ms), "march_ms": float(np.median(march)),
              "march_ms_min": min(march), "march_ms_max": max(march),
              "repeats": args.repeats, "tau_max": float(got[0].max())})
        if (rows, sharing, skips) == (default_rows, 1, 1):
            default = (float(np.median(ms)), got)
    eng.set_tuning(absorption_slab_rows=0, absorption_edge_sharing=1,
                   absorption_skips=1)
    call_ms, (tau, N) = default

    state = None
    if not (args.no_cpu and args.no_baseline):
        state = converged_state.download_state(eng)
        elements = [-1, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5, 5]
        A = np.asarray(eng_abundances(eng, E))
        nH, T, x = state["number_density"], state["temperature"], state["x"]
        n = np.array([nH * (1. if elements[i] < 0 else A[elements[i]]) * x[i]
                      for i in ions])
        b = np.sqrt(np.where(T > 0., 2. * BOLTZMANN * T, 0.)[None, :] /
                    (weights[:, None] * ATOMIC_MASS_UNIT) +
                    2. * SIGMA_TURB * SIGMA_TURB)
    if not args.no_cpu:
        t0 = time.perf_counter()
        rtau, rN = AB.spectra(box, n, b, Sl, gl, origins, d, lengths, nchan,
                              VMIN, VMAX, velocity=vel)
        cpu_ms = 1e3 * (time.perf_counter() - t0)
        # (n and b formed in numpy are a few roundings off the device's:
        # the bound of the engine-cells test, per crossing)
        AD = AB.line_depth(box, n, Sl, dv)[None, :, None]
        bound = (AB.longest_ray * (AD * (3. + 8. * AB.A.U_DEV + AB.DF_EPS) +
                                   2. * rtau) + 26. * rtau) * AB.EPS
        emit({"case": "CPU restatement, %s threads" %
              os.environ.get("OMP_NUM_THREADS", "all"), "ms": cpu_ms,
              "over_the_call": cpu_ms / call_ms,
              "longest_ray": int(AB.longest_ray),
              "difference_over_bound": float(
                  (np.abs(tau - rtau) / np.where(bound > 0., bound, 1.)).max()),
              "column_difference": float(
                  (np.abs(N - rN) / np.where(rN > 0., rN, 1.)).max())})
        del rtau, rN
    if not args.no_baseline:
        zero = np.zeros(box.n)
        g0 = np.zeros(len(names))
        gauss = call(g0)[0]

        def baseline():
            worst = 0.
            for k in range(len(names)):
                for p in range(len(points)):
                    rays = slice(p * per, (p + 1) * per)
                    cube = eng.render_field_absorbing_sky_cube(
                        Sl[k] * n[k], zero, b[k], points[p], d[rays], nchan,
                        VMIN, VMAX, velocity=vel, background=1.)
                    worst = max(worst, float(np.abs(
                        cube.T - np.exp(-gauss[rays, k])).max()))
            return worst

        eng.get_timing(reset=True)
        t0 = time.perf_counter()
        worst = baseline()
        ms = 1e3 * (time.perf_counter() - t0)
        emit({"case": "render_field_absorbing_sky_cube per line and origin "
              "(%d calls, g = 0)" % (len(names) * len(points)), "ms": ms,
              "march_ms": eng.get_timing(reset=True)["kernel_ms"],
              "over_the_call": ms / call_ms,
              "transmission_difference": worst})
    eng.close()
    del backend
    return 0


def eng_abundances(eng, E):
    """He C N O Ne S of the lexington configuration (bench.py)"""
    import bench
    return bench.LEXINGTON_ABUNDANCES


if __name__ == "__main__":
    sys.exit(main())
