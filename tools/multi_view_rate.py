"""Cost of K views in one Monte Carlo run against K single-camera runs
(DESIGN.md 4.11), by the protocol of tools/dust_rate.py: device time of the
dust_shoot_kernel launches (cmi_gpu_get_timing), one warm-up run first.

Workloads:
  galaxy     tests/golden/dust/dusty_galaxy.param (201^3 cells, the spiral
             galaxy source), the parameter file's image; view k of K looks
             along theta = 89.7 deg (1 - k / K), phi = 0
  lexington  H-alpha of a lexingtonHII40 state at 256^3 cells
             (tools/converged_state.py, as tools/scattered_line_rate.py), a
             1024^2 image, dust of 2e-27 m^2 per hydrogen nucleus; view k of
             K looks along theta = 60 deg, phi = 30 deg + 360 deg k / K, each
             with the bounding rectangle of its own projection

Per K (--views) one JSON line: the device time of the K-view run, of each of
the K single-camera runs through cmi_gpu_set_ccd_image with the same views,
seed and packets, their sum, and the steps per packet split into the walk and
the views (cmi_gpu_get_dust_view_counters). --repeats N first runs view 0
through the single-camera call N times (the run-to-run spread).
--single-only leaves the K-view calls out, so that the script also runs on a
tree from before they existed (--tree DIR: import the package and the test
helpers from another checkout).

    python tools/multi_view_rate.py --workload galaxy --views 1 4 16 \\
        --out profiles/multi_view/rate.jsonl
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMA, ALBEDO, G, P_L = 2.e-27, 0.54, 0.44, 0.43


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("galaxy", "lexington"),
                    default="galaxy")
    ap.add_argument("--views", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--warmup", type=float, default=1e5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    sys.path.insert(0, os.path.join(tree, "tools"))
    N = int(args.packets)

    if args.workload == "galaxy":
        import dust_lib
        d = dust_lib.describe(os.path.join(dust_lib.FIXTURES,
                                           "dusty_galaxy.param"),
                              tempfile.mkdtemp())
        eng = dust_lib.make_engine(d, dust_lib.galaxy_density(d))
        img = d["image"]
        nx, ny = img["width"], img["height"]
        backend = None

        def views_of(K):
            return [(img["theta"] * (1. - k / K), img["phi"],
                     tuple(img["anchor"]), tuple(img["sides"]))
                    for k in range(K)]
    else:
        import converged_state
        import line_image_lib as L
        from cmacionize_amd import STROMGREN as box_of
        backend = converged_state.lexington_state(args.ncell, 8, 10000000)
        eng = backend.engine
        eng.synchronize()
        box = L.Box(box_of["anchor"], box_of["sides"], (args.ncell,) * 3)
        nx = ny = args.pixels
        eng.set_dust_scattering_per_hydrogen(G, P_L, ALBEDO, SIGMA)
        eng.set_ccd_image(1., 0.5, nx, ny, (-1., -1.), (2., 2.))
        eng.set_cell_source_line("HAlpha")

        def views_of(K):
            out = []
            for k in range(K):
                theta = np.radians(60.)
                phi = np.radians(30.) + 2. * np.pi * k / K
                anchor, sides = L.bounding_rectangle(box, theta, phi)
                out.append((theta, phi, tuple(anchor), tuple(sides)))
            return out

    def run():
        """one timed run of N packets with the camera that is set"""
        eng.reset_image()
        eng.get_timing(reset=True)
        eng.dust_shoot(args.seed, 0, N)
        eng.synchronize()
        t = eng.get_timing(reset=True)
        c = eng.get_dust_counters()
        assert c["npackets"] == N and c["ncapped"] == 0
        return 1e-3 * t["shoot_ms"], int(t["shoot_launches"]), c

    def single(view):
        eng.set_ccd_image(view[0], view[1], nx, ny, view[2], view[3])
        return run()

    rows = []
    base = {"workload": args.workload, "packets": N, "pixels": [nx, ny],
            "tree": os.path.relpath(tree, ROOT)}
    first = views_of(1)[0]
    eng.set_ccd_image(first[0], first[1], nx, ny, first[2], first[3])
    eng.dust_shoot(args.seed, 0, int(args.warmup))
    eng.synchronize()
    if args.repeats:
        times = []
        for _ in range(args.repeats):
            seconds, launches, c = single(first)
            times.append(seconds)
        rows.append(dict(base, what="single camera, view 0, repeated",
                         device_seconds=times, launches=launches,
                         median=float(np.median(times)),
                         spread=(max(times) - min(times)) / np.median(times),
                         steps_per_packet=c["nsteps"] / N,
                         steps_per_s=c["nsteps"] / float(np.median(times)),
                         scatterings_per_packet=c["nscatter"] / N))
    for K in args.views:
        views = views_of(K)
        row = dict(base, what="K views", K=K)
        singles = [single(v) for v in views]
        row["single_seconds"] = [s[0] for s in singles]
        row["single_seconds_sum"] = sum(s[0] for s in singles)
        row["single_steps_per_packet"] = [s[2]["nsteps"] / N for s in singles]
        if not args.single_only:
            eng.set_ccd_images([v[0] for v in views], [v[1] for v in views],
                               nx, ny, [v[2] for v in views],
                               [v[3] for v in views])
            # (a first short run of the new kernel, as the warm-up above)
            eng.dust_shoot(args.seed, 0, int(args.warmup))
            seconds, launches, c = run()
            per_view = [eng.get_dust_view_counters(v)["nsteps"]
                        for v in range(K)]
            walk = c["nsteps"] - sum(per_view)
            row.update({
                "multi_seconds": seconds, "multi_launches": launches,
                "multi_over_singles": seconds / row["single_seconds_sum"],
                "multi_over_one_single": seconds / singles[0][0],
                "steps_per_packet": c["nsteps"] / N,
                "walk_steps_per_packet": walk / N,
                "view_steps_per_packet": [s / N for s in per_view],
                "steps_per_s": c["nsteps"] / seconds,
                "atomics_per_s": c["natomics"] / seconds,
                "scatterings_per_packet": c["nscatter"] / N})
        rows.append(row)
    eng.close()
    del backend
    for row in rows:
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, "a") as out:
                out.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
