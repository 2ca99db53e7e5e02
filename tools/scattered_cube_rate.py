"""Rate of the scattered-light line cubes on the case of
tools/scattered_line_rate.py: H-alpha of a lexingtonHII40 state at 256^3 cells,
1e7 packets from the cell-luminosity source through dust of 2e-27 m^2 per
hydrogen nucleus (albedo 0.54, g 0.44, p_l 0.43), a 1024^2 image from theta =
60 deg, phi = 30 deg. The same build runs the image mode (the baseline: its
kernel is the parent's, profiles/scattered_cubes/asm_comparison.txt) and the
cube mode with 64 channels over +-60 km/s, the gas expanding radially with 20
km/s at the box's half side and sigma_turb = 5 km/s.

One JSON line on stdout, appended to --out: per mode packets/s, DDA steps/s,
atomics/s and atomics per packet; the cube mode's cost relative to the image
mode; how far its atomics are from 2.35e10 requests/s; the CPU
restatement's packets/s (tests/support/scattered_cube_reference.c over
OMP_NUM_THREADS threads, on --cpu-pixels^2 pixels: its threads each hold a
private cube). CMI_GPU_LIBRARY selects another build of the library (make
variant NAME=lane DEFS=-DCMI_DUST_CUBE_LANE_PER_EVENT); --label names the row.
Every mode is timed --repeats times; the row's figures are the median run's.
--once shoots --packets packets in cube mode once and prints nothing else: to
be run under `rocprofv3 --kernel-trace --stats`.

    python tools/scattered_cube_rate.py --out profiles/scattered_cubes/rate.jsonl
    python tools/scattered_cube_rate.py --ncell 64 --pixels 256 --packets 1e6
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
import scattered_cube_lib as Q  # noqa: E402
import scattered_line_lib as S  # noqa: E402

LINE = "HAlpha"
VIEW = (np.radians(60.), np.radians(30.))
SIGMA, ALBEDO, G, P_L = 2.e-27, 0.54, 0.44, 0.43
NCHAN, VMIN, VMAX = 64, -6.0e4, 6.0e4
EXPANSION, SIGMA_TURB = 2.0e4, 5.0e3
ATOMIC_PEAK = 2.35e10  # fp64 atomic requests/s, DESIGN.md 4.1


def expansion(box):
    """(3, ncell): EXPANSION m/s at the half side, radially from the centre"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in box.ncell],
                               indexing="ij"), axis=0).reshape(3, -1)
    half = 0.5 * np.asarray(box.sides)[:, None]
    mid = (idx + 0.5) / np.asarray(box.ncell)[:, None] * 2. * half - half
    return np.ascontiguousarray(EXPANSION * mid / half.max())


def shoot(eng, seed, n, warmup, repeats):
    eng.dust_shoot(seed, 0, int(warmup))
    eng.get_dust_counters()
    runs = []
    for _ in range(repeats):
        eng.reset_image()
        t0 = time.perf_counter()
        eng.dust_shoot(seed, 0, n)
        c = eng.get_dust_counters()  # waits for the last launch
        runs.append(time.perf_counter() - t0)
        assert c["npackets"] == n and c["ncapped"] == 0
    seconds = float(np.median(runs))
    return {"seconds": seconds, "seconds_of_each_run": runs,
            "packets_per_s": n / seconds,
            "steps_per_s": c["nsteps"] / seconds,
            "steps_per_packet": c["nsteps"] / n,
            "scatterings_per_packet": c["nscatter"] / n,
            "atomics": c["natomics"], "atomics_per_s": c["natomics"] / seconds,
            "atomics_per_packet": c["natomics"] / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--state-packets", type=float, default=1e7)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--warmup", type=float, default=1e5)
    ap.add_argument("--cpu-packets", type=float, default=2e5)
    ap.add_argument("--cpu-pixels", type=int, default=256)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=3,
                    help="timed runs per mode; the row holds the median run "
                         "and every run's seconds")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--label", default="cooperative")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import converged_state
    from cmacionize_amd import STROMGREN as box_of
    from cmacionize_amd import engine as E
    backend = converged_state.lexington_state(args.ncell, args.iterations,
                                              int(args.state_packets))
    eng = backend.engine
    eng.synchronize()
    box = L.Box(box_of["anchor"], box_of["sides"], (args.ncell,) * 3)
    theta, phi = VIEW
    n = args.pixels
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    velocity = expansion(box)
    eng.set_dust_scattering_per_hydrogen(G, P_L, ALBEDO, SIGMA)
    eng.set_ccd_image(theta, phi, n, n, anchor, sides)
    eng.set_cell_velocities(velocity)
    eng.set_cell_source_line(LINE)
    N = int(args.packets)
    if args.once:
        eng.set_scattered_cube(NCHAN, VMIN, VMAX, SIGMA_TURB)
        eng.dust_shoot(args.seed, 0, N)
        eng.get_dust_counters()
        eng.close()
        return 0

    image_mode = shoot(eng, args.seed, N, args.warmup, args.repeats)
    image = eng.download_image()
    eng.set_scattered_cube(NCHAN, VMIN, VMAX, SIGMA_TURB)
    cube_mode = shoot(eng, args.seed, N, args.warmup, args.repeats)
    cube_image = eng.download_image()
    spectrum = eng.download_cubes()[0, 0].sum(axis=(1, 2))
    assert np.allclose(cube_image, image, rtol=1e-9,
                       atol=1e-12 * image[0].max())
    row = {"label": args.label,
           "library": os.path.basename(
               os.environ.get("CMI_GPU_LIBRARY", "libcmi_gpu.so")),
           "ncell": args.ncell, "pixels": n, "line": LINE, "packets": N,
           "nchan": NCHAN, "vmin": VMIN, "vmax": VMAX,
           "expansion": EXPANSION, "sigma_turb": SIGMA_TURB,
           "image_mode": image_mode, "cube_mode": cube_mode,
           "cube_over_image_seconds":
               cube_mode["seconds"] / image_mode["seconds"],
           "cube_atomics_over_peak": cube_mode["atomics_per_s"] / ATOMIC_PEAK,
           "spectrum_fraction_in_axis":
               float(spectrum.sum() / cube_image[0].sum()),
           "channels_lit": int(np.count_nonzero(spectrum))}
    if not args.no_cpu:
        w = eng.compute_emissivities([LINE])[LINE]
        density = eng.download_field(E.FIELD_NUMBER_DENSITY)
        temperature = eng.download_field(E.FIELD_TEMPERATURE)
        m = args.cpu_pixels
        model = S.Model(box.anchor, box.sides, box.ncell, density, SIGMA,
                        ALBEDO, G, P_L, theta, phi, m, m, anchor, sides)
        widths = np.sqrt(2. * (Q.BOLTZMANN * temperature /
                               (Q.HYDROGEN * Q.ATOMIC_MASS_UNIT) +
                               SIGMA_TURB ** 2))
        q = Q.Cube(NCHAN, VMIN, VMAX, widths, SIGMA_TURB, velocity.T)
        ref = Q.Restatement(model, w, q)
        M = int(args.cpu_packets)
        t0 = time.perf_counter()
        _, _, cc = ref.shoot(args.seed, 0, M)
        cpu_seconds = time.perf_counter() - t0
        row.update({"cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                    "cpu_packets": M, "cpu_pixels": m,
                    "cpu_seconds": cpu_seconds,
                    "cpu_packets_per_s": M / cpu_seconds,
                    "speedup": cube_mode["packets_per_s"] /
                    (M / cpu_seconds)})
    eng.close()
    del backend
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as out:
            out.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
