"""Rate of the scattered-light line images: H-alpha of a lexingtonHII40 state
at 256^3 cells (warmed up on the device, tools/converged_state.py, as
tools/line_image_rate.py does), 1e7 packets from the cell-luminosity source
through dust of 2e-27 m^2 per hydrogen nucleus (albedo 0.54, g 0.44, p_l
0.43), peeled off into a 1024^2 image seen from theta = 60 deg, phi = 30 deg.

One JSON line on stdout, appended to --out:
  table_build_ms      cmi_gpu_set_cell_source_line, the whole synchronous call
                      (emissivities, check, cell sums, the host's pass over
                      the block totals): median, min, max of --repeats calls
  gpu_packets_per_s, gpu_steps_per_s, scatterings_per_packet,
  image_atomics_per_s of the run of --packets packets (one warm-up run of
                      --warmup packets first)
  cpu_packets_per_s   the CPU restatement (tests/support/
                      scattered_line_reference.c, OpenMP over OMP_NUM_THREADS
                      threads) on --cpu-packets packets of the same model
  gpu_beats_cpu       the exit status is 1 if it does not

    python tools/scattered_line_rate.py --out profiles/scattered_lines/rate.jsonl
    python tools/scattered_line_rate.py --ncell 64 --pixels 256 --packets 1e6
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

LINE = "HAlpha"
VIEW = (np.radians(60.), np.radians(30.))
SIGMA, ALBEDO, G, P_L = 2.e-27, 0.54, 0.44, 0.43


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--state-packets", type=float, default=1e7)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--warmup", type=float, default=1e5)
    ap.add_argument("--cpu-packets", type=float, default=2e5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import converged_state
    from cmacionize_amd import STROMGREN as box_of
    from cmacionize_amd import engine as E
    t0 = time.perf_counter()
    backend = converged_state.lexington_state(args.ncell, args.iterations,
                                              int(args.state_packets))
    eng = backend.engine
    eng.synchronize()
    print("state: %d^3 after %d iterations of %g packets, %.1f s" %
          (args.ncell, args.iterations, args.state_packets,
           time.perf_counter() - t0), file=sys.stderr)
    box = L.Box(box_of["anchor"], box_of["sides"], (args.ncell,) * 3)
    theta, phi = VIEW
    n = args.pixels
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    eng.set_dust_scattering_per_hydrogen(G, P_L, ALBEDO, SIGMA)
    eng.set_ccd_image(theta, phi, n, n, anchor, sides)

    build_ms = []
    for _ in range(args.repeats + 1):
        t0 = time.perf_counter()
        eng.set_cell_source_line(LINE)
        build_ms.append(1e3 * (time.perf_counter() - t0))
    build_ms = build_ms[1:]
    total = eng.get_cell_source(tables=False)

    eng.dust_shoot(args.seed, 0, int(args.warmup))
    eng.get_dust_counters()
    eng.reset_image()
    N = int(args.packets)
    t0 = time.perf_counter()
    eng.dust_shoot(args.seed, 0, N)
    c = eng.get_dust_counters()  # waits for the last launch
    seconds = time.perf_counter() - t0
    image = eng.download_image()
    assert c["npackets"] == N and c["ncapped"] == 0
    row = {"ncell": args.ncell, "pixels": n, "line": LINE,
           "theta_deg": float(np.degrees(theta)),
           "phi_deg": float(np.degrees(phi)), "sigma": SIGMA,
           "albedo": ALBEDO, "g": G, "p_l": P_L, "packets": N,
           "total_luminosity_W": total,
           "table_build_ms_median": float(np.median(build_ms)),
           "table_build_ms_min": min(build_ms),
           "table_build_ms_max": max(build_ms),
           "gpu_seconds": seconds, "gpu_packets_per_s": N / seconds,
           "steps": c["nsteps"], "gpu_steps_per_s": c["nsteps"] / seconds,
           "steps_per_packet": c["nsteps"] / N,
           "scatterings_per_packet": c["nscatter"] / N,
           "image_atomics": c["natomics"],
           "image_atomics_per_s": c["natomics"] / seconds,
           "lit_pixels": int(np.count_nonzero(image[0])),
           "polarised_fraction": float(
               np.hypot(image[1], image[2]).sum() / image[0].sum())}
    slower = False
    if not args.no_cpu:
        w = eng.compute_emissivities([LINE])[LINE]
        density = eng.download_field(E.FIELD_NUMBER_DENSITY)
        model = S.Model(box.anchor, box.sides, box.ncell, density, SIGMA,
                        ALBEDO, G, P_L, theta, phi, n, n, anchor, sides)
        ref = S.Restatement(model, w)
        assert ref.status == 0
        M = int(args.cpu_packets)
        t0 = time.perf_counter()
        _, cc = ref.shoot(args.seed, 0, M)
        cpu_seconds = time.perf_counter() - t0
        row.update({"cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                    "cpu_packets": M, "cpu_seconds": cpu_seconds,
                    "cpu_packets_per_s": M / cpu_seconds,
                    "cpu_steps_per_s": cc[0] / cpu_seconds,
                    "cpu_steps_per_packet": cc[0] / M,
                    "speedup": (N / seconds) / (M / cpu_seconds),
                    "gpu_beats_cpu": N / seconds > M / cpu_seconds})
        slower = not row["gpu_beats_cpu"]
    eng.close()
    del backend
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as out:
            out.write(line + "\n")
    if slower:
        print("the GPU does not beat the restatement", file=sys.stderr)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
