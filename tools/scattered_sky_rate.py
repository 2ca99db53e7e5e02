"""Rate of the scattered-light sky maps: H-alpha of the lexingtonHII40 state of
tools/scattered_line_rate.py (256^3 cells, warmed up on the device), the
same dust (2e-27 m^2 per hydrogen nucleus, albedo 0.54, g 0.44, p_l 0.43),
1e7 packets from the cell-luminosity source peeled off towards an observer in
the box into a 2048 x 1024 full-sky map. Two observers, those of
tools/sky_map_rate.py: the centre of the box and the centre of one corner
cell; the exclusion radius is one cell side. The parallel camera of
tools/scattered_line_rate.py (its view, its 1024^2 image) is measured on the
same state in the same process, for comparison.

One JSON line per case on stdout, appended to --out:
  gpu_packets_per_s, gpu_steps_per_s, steps_per_packet,
  scatterings_per_packet, image_atomics_per_packet, excluded_events,
  events_outside_the_window of the run of --packets packets (one warm-up run
                      of --warmup packets first)
  cpu_packets_per_s   the CPU restatement (tests/support/
                      scattered_sky_reference.c, OpenMP over OMP_NUM_THREADS
                      threads) on --cpu-packets packets of the same model
The exit status is 1 if the GPU does not beat the restatement in a case.

    python tools/scattered_sky_rate.py --out profiles/scattered_sky/rate.jsonl
    python tools/scattered_sky_rate.py --ncell 64 --nlon 256 --packets 1e6
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
import scattered_sky_lib as K  # noqa: E402

LINE = "HAlpha"
VIEW = (np.radians(60.), np.radians(30.))
SIGMA, ALBEDO, G, P_L = 2.e-27, 0.54, 0.44, 0.43


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--nlon", type=int, default=2048)
    ap.add_argument("--pixels", type=int, default=1024,
                    help="of the parallel camera's image")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--state-packets", type=float, default=1e7)
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--warmup", type=float, default=1e5)
    ap.add_argument("--cpu-packets", type=float, default=2e5)
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
    side = float(box.sides[0]) / args.ncell
    theta, phi = VIEW
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    nlon, nlat = args.nlon, args.nlon // 2
    centre = box.anchor + 0.5 * box.sides
    corner = box.anchor + 0.5 * side
    cases = [("parallel camera", None),
             ("centre", K.Camera(centre, nlon, nlat, side)),
             ("corner cell", K.Camera(corner, nlon, nlat, side))]
    eng.set_dust_scattering_per_hydrogen(G, P_L, ALBEDO, SIGMA)
    eng.set_cell_source_line(LINE)
    N, M = int(args.packets), int(args.cpu_packets)
    w = density = None
    if not args.no_cpu:
        w = eng.compute_emissivities([LINE])[LINE]
        density = eng.download_field(E.FIELD_NUMBER_DENSITY)
    model = S.Model(box.anchor, box.sides, box.ncell,
                    density if density is not None else np.ones(box.n), SIGMA,
                    ALBEDO, G, P_L, theta, phi, args.pixels, args.pixels,
                    anchor, sides)
    slower = False
    for name, cam in cases:
        if cam is None:
            eng.set_ccd_image(theta, phi, args.pixels, args.pixels, anchor,
                              sides)
        else:
            cam.apply(eng)
        eng.dust_shoot(args.seed, 0, int(args.warmup))
        eng.get_dust_counters()
        eng.reset_image()
        t0 = time.perf_counter()
        eng.dust_shoot(args.seed, 0, N)
        c = eng.get_dust_counters()  # waits for the last launch
        seconds = time.perf_counter() - t0
        s = eng.get_sky_camera_counters()
        image = eng.download_image()
        assert c["npackets"] == N and c["ncapped"] == 0
        row = {"case": name, "ncell": args.ncell, "line": LINE,
               "image": list(image.shape[1:]), "sigma": SIGMA,
               "albedo": ALBEDO, "g": G, "p_l": P_L, "packets": N,
               "exclusion_radius_cells": 1 if cam else None,
               "gpu_seconds": seconds, "gpu_packets_per_s": N / seconds,
               "steps": c["nsteps"], "gpu_steps_per_s": c["nsteps"] / seconds,
               "steps_per_packet": c["nsteps"] / N,
               "scatterings_per_packet": c["nscatter"] / N,
               "image_atomics_per_packet": c["natomics"] / N,
               "excluded_events": s["nexcluded"],
               "events_outside_the_window": s["noutside"],
               "lit_pixels": int(np.count_nonzero(image[0])),
               "polarised_fraction": float(
                   np.hypot(image[1], image[2]).sum() / image[0].sum())}
        if not args.no_cpu:
            t0 = time.perf_counter()
            if cam is None:
                ref = S.Restatement(model, w)
                _, cc = ref.shoot(args.seed, 0, M)
            else:
                ref = K.Restatement(model, w, cam)
                _, cc = ref.shoot(args.seed, 0, M)
            cpu_seconds = time.perf_counter() - t0
            row.update({"cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                        "cpu_packets": M, "cpu_seconds": cpu_seconds,
                        "cpu_packets_per_s": M / cpu_seconds,
                        "cpu_steps_per_packet": cc[0] / M,
                        "speedup": (N / seconds) / (M / cpu_seconds),
                        "gpu_beats_cpu": N / seconds > M / cpu_seconds})
            slower = slower or not row["gpu_beats_cpu"]
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, "a") as out:
                out.write(line + "\n")
    eng.close()
    del backend
    if slower:
        print("the GPU does not beat the restatement", file=sys.stderr)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
