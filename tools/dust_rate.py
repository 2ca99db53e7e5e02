"""Packet rate of the dusty radiative transfer mode on dusty_galaxy.param
(201^3 cells): shoots N packets through the C ABI and prints packets/s, DDA
steps/s, mean scatterings per packet and image atomics/s (device time of the
dust_shoot_kernel launches). --cpu N: the same for the CPU restatement
(tests/support/dust_reference.c, OpenMP over OMP_NUM_THREADS threads) on N
packets.

    python tools/dust_rate.py --packets 1e7 1e8
    python tools/dust_rate.py --cpu 2e5
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dust_lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=float, nargs="*", default=[1e7, 1e8])
    ap.add_argument("--cpu", type=float, default=0.)
    ap.add_argument("--params", default=os.path.join(dust_lib.FIXTURES,
                                                     "dusty_galaxy.param"))
    args = ap.parse_args()
    d = dust_lib.describe(args.params, tempfile.mkdtemp())
    density = dust_lib.galaxy_density(d)
    seed = d["random_seed"]
    if args.cpu:
        n = int(args.cpu)
        ref = dust_lib.Restatement(d, density)
        t0 = time.perf_counter()
        _, c = ref.shoot(seed, 0, n)
        dt = time.perf_counter() - t0
        print(json.dumps({"side": "cpu", "threads": os.environ.get(
            "OMP_NUM_THREADS"), "packets": n, "seconds": dt,
            "packets_per_s": n / dt, "steps_per_s": c[0] / dt,
            "scatterings_per_packet": c[1] / n}))
        return
    eng = dust_lib.make_engine(d, density)
    eng.dust_shoot(seed, 0, 100000)  # warm-up
    eng.synchronize()
    for n in args.packets:
        n = int(n)
        eng.reset_image()
        eng.get_timing(reset=True)
        t0 = time.perf_counter()
        eng.dust_shoot(seed, 0, n)
        eng.synchronize()
        wall = time.perf_counter() - t0
        ms = eng.get_timing(reset=True)["shoot_ms"]
        c = eng.get_dust_counters()
        dt = ms * 1e-3
        print(json.dumps({"side": "gpu", "packets": n, "device_seconds": dt,
                          "wall_seconds": wall, "packets_per_s": n / dt,
                          "steps_per_s": c["nsteps"] / dt,
                          "scatterings_per_packet": c["nscatter"] / n,
                          "atomics_per_s": c["natomics"] / dt,
                          "capped": c["ncapped"]}))
    eng.close()


if __name__ == "__main__":
    main()
