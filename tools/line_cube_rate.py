"""Rate of the spectral line cubes: H alpha at 1024^2 pixels and 64 velocity
channels of a lexingtonHII40 state at 256^3 cells (warmed up on the device,
tools/converged_state.py) with a radial expansion v = v0 r / r0 about the
centre, for the views theta = 0 and theta = 60 deg, phi = 30 deg, without and
with dust.

Per case: milliseconds of the whole synchronous call (records, the march per
block of channels, the cube's copy to the host; one warm-up, then --repeats
calls: median, min, max), and the same case on the CPU restatement
(tests/support/line_cube_reference.c, OpenMP over OMP_NUM_THREADS threads),
fed with the device's emissivities and widths computed in numpy. One JSON
line per case on stdout and appended to --out.

The split between the record and the march kernel needs a run of its own:
--once renders the first case once, to be run under
`rocprofv3 --kernel-trace --stats`. CMI_GPU_LIBRARY selects another build of
the library (make variant NAME=cb16 DEFS=-DCMI_LINE_CUBE_CB=16) for the
comparison of channel blocks. --table FILE prints the lines of a jsonl file
as the table of DESIGN.md 4.12 and does nothing else. --erf measures the
device's erf against glibc's (the U_DEV of tests/test_gpu_line_cube.py) and
does nothing else.

    python tools/line_cube_rate.py --out profiles/line_cubes/rate.jsonl
    python tools/line_cube_rate.py --ncell 64 --pixels 256 --no-cpu
    python tools/line_cube_rate.py --table profiles/line_cubes/rate.jsonl
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

import line_cube_lib as Q  # noqa: E402
import line_image_lib as L  # noqa: E402

LINE = "HAlpha"
VIEWS = [(0., 0.), (np.radians(60.), np.radians(30.))]
SIGMA = 2.e-27  # m^2 per H: optical depth ~6 through 10 pc of 1e8 m^-3
V0 = 20.e3      # m s^-1 at the box's half side
VMIN, VMAX = -60.e3, 60.e3
K_B, M_U = 1.38064852e-23, 1.660539040e-27


def table(path):
    print("| view | dust | channels | GPU ms (min .. max) | crossings | "
          "CPU ms | GPU / CPU | worst difference / I_tot |")
    print("|---|---|---|---|---|---|---|---|")
    for line in open(path):
        r = json.loads(line)
        print("| %g, %g | %s | %d | %.1f (%.1f .. %.1f) | %s | %s | %s | %s |"
              % (r["theta_deg"], r["phi_deg"], "yes" if r["dust"] else "no",
                 r["channels"], r["gpu_ms_median"], r["gpu_ms_min"],
                 r["gpu_ms_max"],
                 "%.3g" % r["crossings"] if "crossings" in r else "-",
                 "%.0f" % r["cpu_ms"] if "cpu_ms" in r else "-",
                 "%.1f" % r["speedup"] if "speedup" in r else "-",
                 "%.2g" % r["worst_difference"] if "worst_difference" in r
                 else "-"))


def measure_erf(n=1000):
    """The device's clamped erf against glibc's at n^2 points of [-6, 6],
    through render_field_cube on single-cell rays: a slab of n x n x 1 unit
    cells seen along z, q = 1 and ds = 1 exactly, one channel [-12, 0): the
    pixel of a cell with u is 0.5 * (E(-u) + 1)."""
    from cmacionize_amd import GpuEngine
    box = L.Box((0., 0., 0.), (float(n), float(n), 1.), (n, n, 1))
    eng = GpuEngine((n, n, 1), tuple(box.anchor), tuple(box.sides), (0, 0, 0),
                    device=0)
    u = np.random.default_rng(1).uniform(-6., 6., box.n)
    vel = np.zeros((3, box.n))
    vel[2] = -u
    j = np.full(box.n, 4. * np.pi)
    b = np.ones(box.n)
    anchor, sides = L.bounding_rectangle(box, 0., 0.)
    got = eng.render_field_cube(j, b, 0., 0., n, n, anchor, sides, 1, -12.,
                                0., velocity=vel)[0, 0]
    want = Q.render(box, j, b, 0., 0., n, n, anchor, sides, 1, -12., 0.,
                    velocity=vel)[0, 0]
    eng.close()
    eps = np.finfo(float).eps
    err = 2. * np.abs(got - want) / eps
    print("pixels", got.size, "nonzero", int((got > 0).sum()), "min",
          got.min(), "max", got.max())
    print("worst |E_dev - E_cpu| in eps:", err.max(), "mean", err.mean())
    print("pixels that differ:", int((got != want).sum()))
    # in ulps of erf itself, where 2 f - 1 is exact (|erf| >= 0.5)
    e_dev, e_cpu = 2. * got - 1., 2. * want - 1.
    big = np.abs(e_cpu) >= 0.5
    print("worst in ulps of erf where |erf| >= 0.5:",
          (np.abs(e_dev - e_cpu)[big] / np.spacing(np.abs(e_cpu[big]))).max())
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--erf", action="store_true")
    ap.add_argument("--table", default=None)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=64)
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
    if args.erf:
        return measure_erf()

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
    # v = V0 r / r0 about the centre of the box, r0 its half side
    centre = box.anchor + 0.5 * box.sides
    axes = [box.anchor[a] + (np.arange(args.ncell) + 0.5) * box.cellside[a] -
            centre[a] for a in range(3)]
    r = np.stack(np.meshgrid(*axes, indexing="ij")).reshape(3, -1)
    vel = V0 * r / (0.5 * box.sides[:, None])
    del r
    eng.set_cell_velocities(vel)
    j = widths = density = None
    if not args.no_cpu and not args.once:
        j = eng.compute_emissivities([LINE])[LINE]
        density = eng.download_field(E.FIELD_NUMBER_DENSITY)
        temperature = eng.download_field(E.FIELD_TEMPERATURE)
        widths = np.sqrt(2. * K_B * temperature /
                         (E.LINE_ATOMIC_WEIGHTS[LINE] * M_U))
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a")
    for theta, phi in VIEWS:
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        for sigma in (0., SIGMA):
            call = lambda: eng.render_line_cube(
                [LINE], theta, phi, n, n, anchor, sides, nchan, VMIN, VMAX, 1,
                sigma)[LINE]
            cube = call()  # warm-up
            if args.once:
                return 0
            ms = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                cube = call()
                ms.append(1e3 * (time.perf_counter() - t0))
            row = {"ncell": args.ncell, "pixels": n, "channels": nchan,
                   "line": LINE, "library": os.path.basename(E.LIB_PATH),
                   "theta_deg": float(np.degrees(theta)),
                   "phi_deg": float(np.degrees(phi)), "dust": sigma > 0.,
                   "gpu_ms_median": float(np.median(ms)),
                   "gpu_ms_min": min(ms), "gpu_ms_max": max(ms),
                   "repeats": args.repeats}
            if j is not None:
                ext = density * sigma if sigma else None
                t0 = time.perf_counter()
                ref = Q.render(box, j, widths, theta, phi, n, n, anchor,
                               sides, nchan, VMIN, VMAX, 1, extinction=ext,
                               velocity=vel)[0]
                cpu_ms = 1e3 * (time.perf_counter() - t0)
                total = L.render(box, j, theta, phi, n, n, anchor, sides, 1,
                                 extinction=ext)[0]
                lit = total > 0.
                row.update({
                    "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                    "cpu_ms": cpu_ms, "crossings": Q.last_crossings,
                    "speedup": cpu_ms / row["gpu_ms_median"],
                    "worst_difference": float(
                        (np.abs(cube - ref)[:, lit] / total[lit]).max())})
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
