"""Cost of the Lyman-alpha radiation field on the case of
tools/lyman_alpha_rate.py - the converged lexingtonHII40 state, its own H I,
radial expansion, no dust, one --pixels^2 view of 64 channels, core skipping at
--x-crit -: --repeats timed runs of --packets packets with the field off and
with it on, alternating in one process (off, on, off, on, ...).

One JSON line per mode on stdout, appended to --out: the seconds of each run,
their median, packets/s, crossings/s, and for the field its sums (sum L, sum
S_H, sum N_H). A library without the field (the parent commit's, selected with
CMI_GPU_LIBRARY) gives the "off" line alone; --label names the rows.

With --sphere the static sphere of the tests instead (lyman_alpha_lib.
sphere_scene: a tau_0 = 1000, 10 K, 24^3 cells): the force multiplier M_F =
sum_c G_c . r_hat_c / npackets - the momentum the gas takes up in units of
L / c - next to 3.51 (a tau_0)^(1/3) of Dijkstra & Loeb (2008), at --x-crit.

    python tools/lya_field_rate.py --out profiles/lya_field/rate.jsonl
    python tools/lya_field_rate.py --sphere --x-crit 0 --packets 1000
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
import lyman_alpha_rate as R  # noqa: E402


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def sphere(args):
    import lyman_alpha_lib as Y
    scene, b, a = Y.sphere_scene()
    scene.x_crit = args.x_crit
    eng = scene.engine()
    eng.set_lya_field()
    N = int(args.packets)
    t0 = time.perf_counter()
    eng.lya_shoot(args.seed, 0, N)
    c = eng.get_lya_counters()
    seconds = time.perf_counter() - t0
    f = eng.download_lya_field()
    eng.close()
    m = scene.m
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in m.ncell],
                               indexing="ij"), axis=-1).reshape(-1, 3)
    r = m.anchor + (idx + 0.5) * (m.sides / m.ncell)
    r_hat = r / np.sqrt((r * r).sum(axis=1))[:, None]
    G = np.stack([f["G_x"], f["G_y"], f["G_z"]], axis=1)
    emit({"label": args.label, "case": "static sphere",
          "a_tau0": Y.SPHERE_A_TAU0, "ncell": int(m.ncell[0]), "packets": N,
          "x_crit": args.x_crit, "seconds": seconds,
          "scatterings_per_packet": c["nhydrogen"] / N,
          "capped": c["ncapped"],
          "force_multiplier": float((G * r_hat).sum() / N),
          "dijkstra_loeb_2008": 3.51 * Y.SPHERE_A_TAU0 ** (1. / 3.),
          "sum_S_H_per_packet": float(f["S_H"].sum() / N),
          "sum_N_H_per_packet": float(f["N_H"].sum() / N)}, args.out)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--pixels", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--state-packets", type=float, default=1e7)
    ap.add_argument("--packets", type=float, default=5e4)
    ap.add_argument("--warmup", type=float, default=1e3)
    ap.add_argument("--x-crit", type=float, default=10.)
    ap.add_argument("--max-scatter", type=float, default=1e7)
    ap.add_argument("--floor-temperature", type=float, default=100.)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sphere", action="store_true")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.sphere:
        return sphere(args)

    import converged_state
    from cmacionize_amd import STROMGREN as box_of
    from cmacionize_amd import engine as E
    backend = converged_state.lexington_state(args.ncell, args.iterations,
                                              int(args.state_packets))
    eng = backend.engine
    eng.synchronize()
    box = L.Box(box_of["anchor"], box_of["sides"], (args.ncell,) * 3)
    theta, phi = R.VIEW
    n = args.pixels
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    density = eng.download_field(E.FIELD_NUMBER_DENSITY)
    temperature = np.maximum(eng.download_field(E.FIELD_TEMPERATURE),
                             args.floor_temperature)
    n_HI = density * eng.download_field(E.FIELD_IONIC_FRACTION)
    eng.set_dust_scattering_per_hydrogen(0.5, 0., 0., 0.)
    eng.set_ccd_image(theta, phi, n, n, anchor, sides)
    eng.set_cell_velocities(R.expansion(box))
    eng.set_cell_source_field(eng.lyman_alpha_emissivity())
    eng.set_lyman_alpha(R.NCHAN, R.VMIN, R.VMAX, 0., args.x_crit,
                        int(args.max_scatter), n_HI, temperature)
    have_field = hasattr(eng._lib, "cmi_gpu_set_lya_field")
    modes = ("off", "on") if have_field else ("off",)
    N = int(args.packets)
    eng.lya_shoot(args.seed, 0, int(args.warmup))
    eng.get_lya_counters()
    runs = {mode: [] for mode in modes}
    sums = {}
    for _ in range(args.repeats):
        for mode in modes:
            if have_field:
                eng.set_lya_field(mode == "on")
            eng.reset_lya()
            t0 = time.perf_counter()
            eng.lya_shoot(args.seed, 0, N)
            c = eng.get_lya_counters()  # waits for the last launch
            runs[mode].append(time.perf_counter() - t0)
            assert c["npackets"] == N
            if mode == "on" and not c["ncapped"]:
                f = eng.download_lya_field()
                sums = {"sum_L": float(f["L"].sum()),
                        "sum_S_H": float(f["S_H"].sum()),
                        "sum_N_H": float(f["N_H"].sum())}
    for mode in modes:
        seconds = float(np.median(runs[mode]))
        row = {"label": args.label, "field": mode,
               "library": os.path.basename(
                   os.environ.get("CMI_GPU_LIBRARY", "libcmi_gpu.so")),
               "ncell": args.ncell, "pixels": n, "packets": N,
               "x_crit": args.x_crit, "max_scatter": int(args.max_scatter),
               "seconds": seconds, "seconds_of_each_run": runs[mode],
               "packets_per_s": N / seconds,
               "crossings_per_s": c["nsteps"] / seconds,
               "scatterings_per_packet":
                   (c["nhydrogen"] + c["ndust"]) / N,
               "crossings_per_packet": c["nsteps"] / N,
               "capped": c["ncapped"]}
        if mode == "on":
            row.update(sums)
        emit(row, args.out)
    eng.close()
    del backend
    return 0


if __name__ == "__main__":
    sys.exit(main())
