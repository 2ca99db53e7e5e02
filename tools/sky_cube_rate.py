"""Rate of the sky cubes: H alpha as a 2048 x 1024 full-sky map of 64 velocity
channels, seen from a point inside a lexingtonHII40 state at 256^3 cells
(warmed up on the device, tools/converged_state.py) with the radial expansion
v = v0 r / r0 about the centre of tools/line_cube_rate.py, without and with
dust.

Per case: milliseconds of the whole synchronous call of
render_line_sky_map_cube (records, directions up, the march per block of
channels, the cube's copy to the host, the reordering of the tiles; one
warm-up, then --repeats calls: median, min, max), next to it the integrated
map (render_line_sky_map) of the same line from the same point on the same
state, and the same rays on the CPU restatement
(tests/support/sky_cube_reference.c, OpenMP over OMP_NUM_THREADS threads), fed
with the device's emissivities and widths computed in numpy. One JSON line
per case on stdout and appended to --out.

The split between the record and the march kernel needs a run of its own:
--once renders the first case once, to be run under
`rocprofv3 --kernel-trace --stats`. CMI_GPU_LIBRARY selects another build of
the library (make variant NAME=skycb16 DEFS=-DCMI_SKY_CUBE_CB=16) for the
comparison of channel blocks. --table FILE prints the lines of a jsonl file
as the table of DESIGN.md 4.13 and does nothing else.

    python tools/sky_cube_rate.py --out profiles/sky_cubes/rate.jsonl
    python tools/sky_cube_rate.py --ncell 64 --nlon 256 --nlat 128 --no-cpu
    python tools/sky_cube_rate.py --table profiles/sky_cubes/rate.jsonl
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

import sky_cube_lib as Q  # noqa: E402
import sky_image_lib as S  # noqa: E402

LINE = "HAlpha"
SIGMA = 2.e-27  # m^2 per H: optical depth ~6 through 10 pc of 1e8 m^-3
V0 = 20.e3      # m s^-1 at the box's half side
VMIN, VMAX = -60.e3, 60.e3
# the observer: fractions of the box sides from the anchor, and a velocity
OBSERVER = (0.3, 0.4, 0.45)
V_OBS = (5.e3, -3.e3, 2.e3)
K_B, M_U = 1.38064852e-23, 1.660539040e-27


def table(path):
    print("| dust | channels | library | cube ms (min .. max) | map ms | "
          "crossings | CPU ms | GPU / CPU | worst difference / I_tot |")
    print("|---|---|---|---|---|---|---|---|---|")
    for line in open(path):
        r = json.loads(line)
        print("| %s | %d | %s | %.1f (%.1f .. %.1f) | %.1f | %s | %s | %s | "
              "%s |"
              % ("yes" if r["dust"] else "no", r["channels"], r["library"],
                 r["gpu_ms_median"], r["gpu_ms_min"], r["gpu_ms_max"],
                 r["map_ms_median"],
                 "%.3g" % r["crossings"] if "crossings" in r else "-",
                 "%.0f" % r["cpu_ms"] if "cpu_ms" in r else "-",
                 "%.1f" % r["speedup"] if "speedup" in r else "-",
                 "%.2g" % r["worst_difference"] if "worst_difference" in r
                 else "-"))


def timed(call, repeats):
    result = call()  # warm-up
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return result, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--nlon", type=int, default=2048)
    ap.add_argument("--nlat", type=int, default=1024)
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
    nlon, nlat, nchan = args.nlon, args.nlat, args.channels
    origin = box.anchor + box.sides * np.array(OBSERVER)
    # v = V0 r / r0 about the centre of the box, r0 its half side
    centre = box.anchor + 0.5 * box.sides
    axes = [box.anchor[a] + (np.arange(args.ncell) + 0.5) * box.cellside[a] -
            centre[a] for a in range(3)]
    r = np.stack(np.meshgrid(*axes, indexing="ij")).reshape(3, -1)
    vel = V0 * r / (0.5 * box.sides[:, None])
    del r
    eng.set_cell_velocities(vel)
    j = widths = density = directions = None
    if not args.no_cpu and not args.once:
        j = eng.compute_emissivities([LINE])[LINE]
        density = eng.download_field(E.FIELD_NUMBER_DENSITY)
        temperature = eng.download_field(E.FIELD_TEMPERATURE)
        widths = np.sqrt(2. * K_B * temperature /
                         (E.LINE_ATOMIC_WEIGHTS[LINE] * M_U))
        directions, _ = E.sky_map_directions(nlon, nlat)
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "a")
    for sigma in (0., SIGMA):
        call = lambda: eng.render_line_sky_map_cube(
            [LINE], origin, nlon, nlat, nchan, VMIN, VMAX,
            dust_cross_section=sigma, observer_velocity=V_OBS)[LINE]
        if args.once:
            call()
            return 0
        cube, ms = timed(call, args.repeats)
        sky, map_ms = timed(lambda: eng.render_line_sky_map(
            [LINE], origin, nlon, nlat, dust_cross_section=sigma)[LINE],
            args.repeats)
        row = {"ncell": args.ncell, "nlon": nlon, "nlat": nlat,
               "channels": nchan, "line": LINE,
               "library": os.path.basename(E.LIB_PATH), "dust": sigma > 0.,
               "gpu_ms_median": float(np.median(ms)), "gpu_ms_min": min(ms),
               "gpu_ms_max": max(ms),
               "map_ms_median": float(np.median(map_ms)),
               "map_ms_min": min(map_ms), "map_ms_max": max(map_ms),
               "channels_sum_over_map": float(cube.sum() / sky.sum()),
               "repeats": args.repeats}
        if j is not None:
            ext = density * sigma if sigma else None
            t0 = time.perf_counter()
            ref = Q.render(box, j, widths, origin, directions, nchan, VMIN,
                           VMAX, extinction=ext, velocity=vel,
                           observer_velocity=V_OBS)[0]
            cpu_ms = 1e3 * (time.perf_counter() - t0)
            total = S.render(box, j, origin, directions, extinction=ext)[0]
            lit = total > 0.
            got = cube.reshape(nchan, -1)
            row.update({
                "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                "cpu_ms": cpu_ms, "crossings": Q.last_crossings,
                "speedup": cpu_ms / row["gpu_ms_median"],
                "worst_difference": float(
                    (np.abs(got - ref)[:, lit] / total[lit]).max())})
            del ref, got
        del cube
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
