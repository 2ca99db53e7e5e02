#!/usr/bin/env python3
"""What the escape tally costs: transport time of one iteration on the
lexingtonHII40 state.

Three ways to fly the same packets of the same iteration, alternating in one
process, `--repeats` timed runs each after one untimed run:

  fast     trackers off: the launch plan every iteration but the last has
  tracker  trackers on, one spectrum tracker in a vacuum cell, which counts
           nothing: the routing a set tally brings (the exact marcher, no
           combining table, no tile rounds) without the tally
  tally    trackers on, the escape tally set (and no tracker)

tally - tracker is the tally's own cost, tally - fast what a user pays in the
last iteration. One JSON line per row goes to stdout and to --out.

The lexington nebula is ionization bounded - about one packet in 10^4 gets
out - so that case says little about the atomics. `--density-scale s`
multiplies the state's densities by s before the timed runs (0.02: a leaky
nebula; 0: a box of vacuum, every packet escapes at once), and `--nlon 1
--nmu 1 --nfreq 1` sends all of them to one address per photon type: the
worst the one-atomic-per-packet baseline can meet.

    python tools/escape_rate.py --out profiles/escape/rate.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from converged_state import lexington_state  # noqa: E402
from cmacionize_amd import engine as E  # noqa: E402


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=3,
                    help="iterations that make the state")
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--nlon", type=int, default=64)
    ap.add_argument("--nmu", type=int, default=32)
    ap.add_argument("--nfreq", type=int, default=16)
    ap.add_argument("--density-scale", type=float, default=1.)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    packets = int(args.packets)
    backend = lexington_state(args.ncell, args.iterations, packets)
    eng = backend.engine
    loop = args.iterations
    if args.density_scale != 1.:
        eng.upload_cells(
            args.density_scale * eng.download_field(E.FIELD_NUMBER_DENSITY),
            eng.download_field(E.FIELD_TEMPERATURE),
            np.array([eng.download_field(E.FIELD_IONIC_FRACTION + i)
                      for i in range(E.NION)]))
    have_tally = hasattr(eng, "set_escape_tally")
    # the centre of lexingtonHII40 is a vacuum ball of radius 3e16 m
    vacuum = [[1.e14, 1.e14, 1.e14]]

    def fly(mode):
        eng.set_spectrum_trackers(vacuum if mode == "tracker" else
                                  np.zeros((0, 3)))
        if have_tally:
            if mode == "tally":
                eng.set_escape_tally(args.nlon, args.nmu, nfreq=args.nfreq)
            else:
                eng.set_escape_tally(0, 0)
        eng.enable_trackers(mode != "fast")
        eng.reset_grid()
        eng.synchronize()
        t0 = time.perf_counter()
        eng.shoot(args.seed, loop, 0, packets)
        eng.synchronize()
        seconds = time.perf_counter() - t0
        tw, tc, nsteps = eng.get_counters()
        row = dict(mode=mode, ms=1e3 * seconds, typecount=list(tc),
                   totweight=tw, dda_steps=int(nsteps))
        if mode == "tally":
            sky = eng.escape_tally()
            row["tally_sums"] = list(sky.sum(axis=(1, 2, 3)))
            row["pixels_in_use"] = int((sky.sum(axis=(0, 1)) > 0).sum())
        return row

    modes = ["fast", "tracker"] + (["tally"] if have_tally else [])
    for mode in modes:
        fly(mode)  # untimed: buffers, the first launch of each build
    rows = {mode: [] for mode in modes}
    for _ in range(args.repeats):
        for mode in modes:
            rows[mode].append(fly(mode))
    for mode in modes:
        last = rows[mode][-1]
        ms = [r["ms"] for r in rows[mode]]
        out = dict(label=args.label, ncell=args.ncell, packets=packets,
                   state_iterations=args.iterations,
                   density_scale=args.density_scale, mode=mode, ms=ms,
                   ms_median=float(np.median(ms)),
                   typecount=last["typecount"], dda_steps=last["dda_steps"])
        if mode == "tally":
            out.update(nlon=args.nlon, nmu=args.nmu, nfreq=args.nfreq,
                       tally_sums=last["tally_sums"],
                       pixels_in_use=last["pixels_in_use"],
                       escape_atomics=float(sum(last["tally_sums"])))
        emit(out, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
