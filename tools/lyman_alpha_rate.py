"""Rate of the Lyman-alpha transfer on a converged lexingtonHII40 state:
packets from the cells' recombination emissivity (lyman_alpha_emissivity)
scatter off the state's own H I (n_H x_H, the cells' temperatures, floored at
--floor-temperature), the gas expanding radially with 20 km/s at the box's half
side, no dust, one --pixels^2 image with 64 channels over +-800 km/s from theta
= 60 deg, phi = 30 deg, core skipping at --x-crit and the cap --max-scatter.

One JSON line on stdout, appended to --out: packets/s, scatterings/s, cell
crossings/s, scatterings and crossings per packet, capped packets, of the
median of --repeats timed runs in one process; with --cpu-packets the CPU
restatement's packets/s (tests/support/lyman_alpha_reference.c over
OMP_NUM_THREADS threads, on --cpu-pixels^2 pixels). CMI_GPU_LIBRARY selects
another build of the library (make variant NAME=events
DEFS=-DCMI_LYA_EVENT_LOOP); --label names the row.

    python tools/lyman_alpha_rate.py --out profiles/lyman_alpha/rate.jsonl
    python tools/lyman_alpha_rate.py --ncell 64 --pixels 128 --packets 2e4
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
import scattered_line_lib as S  # noqa: E402

VIEW = (np.radians(60.), np.radians(30.))
NCHAN, VMIN, VMAX = 64, -8.0e5, 8.0e5
EXPANSION = 2.0e4


def expansion(box):
    """(3, ncell): EXPANSION m/s at the half side, radially from the centre"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in box.ncell],
                               indexing="ij"), axis=0).reshape(3, -1)
    half = 0.5 * np.asarray(box.sides)[:, None]
    mid = (idx + 0.5) / np.asarray(box.ncell)[:, None] * 2. * half - half
    return np.ascontiguousarray(EXPANSION * mid / half.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--state-packets", type=float, default=1e7)
    ap.add_argument("--packets", type=float, default=1e5)
    ap.add_argument("--warmup", type=float, default=1e3)
    ap.add_argument("--x-crit", type=float, default=3.)
    ap.add_argument("--max-scatter", type=float, default=1e6)
    ap.add_argument("--floor-temperature", type=float, default=100.)
    ap.add_argument("--cpu-packets", type=float, default=0.)
    ap.add_argument("--cpu-pixels", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="one packet per lane")
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
    density = eng.download_field(E.FIELD_NUMBER_DENSITY)
    temperature = np.maximum(eng.download_field(E.FIELD_TEMPERATURE),
                             args.floor_temperature)
    x_H = eng.download_field(E.FIELD_IONIC_FRACTION)
    n_HI = density * x_H
    source = eng.lyman_alpha_emissivity()
    eng.set_dust_scattering_per_hydrogen(0.5, 0., 0., 0.)
    eng.set_ccd_image(theta, phi, n, n, anchor, sides)
    eng.set_cell_velocities(velocity)
    eng.set_cell_source_field(source)
    eng.set_lyman_alpha(NCHAN, VMIN, VMAX, 0., args.x_crit,
                        int(args.max_scatter), n_HI, temperature)
    N = int(args.packets)
    eng.lya_shoot(args.seed, 0, int(args.warmup))
    eng.get_lya_counters()
    runs = []
    for _ in range(args.repeats):
        eng.reset_lya()
        t0 = time.perf_counter()
        eng.lya_shoot(args.seed, 0, N)
        c = eng.get_lya_counters()  # waits for the last launch
        runs.append(time.perf_counter() - t0)
        assert c["npackets"] == N
    seconds = float(np.median(runs))
    scatterings = c["nhydrogen"] + c["ndust"]
    row = {"label": args.label,
           "library": os.path.basename(
               os.environ.get("CMI_GPU_LIBRARY", "libcmi_gpu.so")),
           "ncell": args.ncell, "pixels": n, "packets": N,
           "x_crit": args.x_crit, "max_scatter": int(args.max_scatter),
           "floor_temperature": args.floor_temperature,
           "seconds": seconds, "seconds_of_each_run": runs,
           "packets_per_s": N / seconds,
           "scatterings_per_s": scatterings / seconds,
           "crossings_per_s": c["nsteps"] / seconds,
           "scatterings_per_packet": scatterings / N,
           "crossings_per_packet": c["nsteps"] / N,
           "rejections_per_scattering": c["nrejections"] / max(scatterings, 1),
           "atomics": c["natomics"], "capped": c["ncapped"]}
    if args.cpu_packets:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import lyman_alpha_lib as Y
        m = args.cpu_pixels
        model = S.Model(box.anchor, box.sides, box.ncell, density, 0., 0., 0.5,
                        0., theta, phi, m, m, anchor, sides)
        scene = Y.Scene(model, source, n_HI, temperature, NCHAN, VMIN, VMAX,
                        velocity.T, 0., args.x_crit, int(args.max_scatter),
                        dust=False)
        ref = Y.Restatement(scene)
        M = int(args.cpu_packets)
        t0 = time.perf_counter()
        _, _, cc, _ = ref.shoot(args.seed, 0, M)
        cpu_seconds = time.perf_counter() - t0
        row.update({"cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                    "cpu_packets": M, "cpu_pixels": m,
                    "cpu_seconds": cpu_seconds,
                    "cpu_packets_per_s": M / cpu_seconds,
                    "cpu_scatterings_per_packet":
                        (cc["nhydrogen"] + cc["ndust"]) / M,
                    "speedup": (N / seconds) / (M / cpu_seconds)})
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
