#!/usr/bin/env python3
"""GPU box, experiment build (make -C cmacionize_amd/csrc variant NAME=exp
DEFS=-DCMI_EXPERIMENTS; CMI_GPU_LIBRARY=.../libcmi_gpu_exp.so): where the
hydrogen-only first generation spends its time OUTSIDE the march loop's
instruction count - on a fixed converged state of stromgren.param, one launch
with cycle stamps (tuning key phase_stamps, cmi_gpu_get_phase_clocks):

* the share of the waves' cycles in each section of the outer loop: waiting
  at the flush point's first barrier, the flush, the refill, the march loop,
  the end of flights;
* when the blocks leave the kernel, against the launch's end (the tail: the
  SIMDs run at fewer and fewer waves once blocks have gone);
* the kernel's time over the grid sizes --ncell (default 64 128 256): its
  slope per DDA step per packet and its intercept - the part of the kernel
  that does not scale with the march.

    python tools/first_generation_phases.py [--ncell N ...] [--packets P]
        [key=value tuning ...]

The stamps cost time themselves (the launch with stamps is printed next to
the one without); shares, not absolute times, are what this is for.
"""
import argparse
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0] + "/tools")
from run_config import make  # noqa: E402

SECTIONS = ("barrier wait", "flush", "refill", "march", "end of flights")


def first_generation_ms(eng, npk, loop):
    eng.reset_grid()
    eng.get_timing(reset=True)
    eng.shoot(42, loop, 0, npk)
    tw, tc, ns = eng.get_counters()
    first = [ms for ms, pk in eng.get_launch_times() if pk == npk]
    return (first[0] if first else float("nan")), ns / npk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--packets", type=float, default=1e8)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("tuning", nargs="*")
    args = ap.parse_args()
    npk = int(args.packets)
    tuning = {k: int(v) for k, v in (t.split("=") for t in args.tuning)}
    print("tuning:", tuning or "defaults", flush=True)
    points = []
    for ncell in args.ncell:
        eng = make("stromgren", ncell)
        eng.set_tuning(timing=1, **tuning)
        for loop in range(args.iterations):
            eng.reset_grid()
            eng.shoot(42, loop, 0, npk)
            tw, tc, ns = eng.get_counters()
            eng.update_cells(loop, tw)
        plain = [first_generation_ms(eng, npk, args.iterations + 1)
                 for _ in range(3)]
        ms = float(np.median([m for m, _ in plain]))
        steps = plain[0][1]
        points.append((steps, ms))
        # (the counters are those of the last launch: one first generation)
        trips = eng.get_wave_steps()
        print("ncell %d: first generation %.2f ms (%s), %.1f steps/packet, "
              "%.2f lanes stepping per wave iteration, %.4f wave iterations "
              "per packet"
              % (ncell, ms, " ".join("%.2f" % m for m, _ in plain), steps,
                 steps * npk / max(trips, 1), trips / npk),
              flush=True)
        if ncell != args.ncell[-1]:
            eng.close()
            continue
        # the largest grid: one launch with stamps
        eng.set_tuning(phase_stamps=1)
        stamped, _ = first_generation_ms(eng, npk, args.iterations + 1)
        cycles, start, ends = eng.get_phase_clocks()
        eng.set_tuning(phase_stamps=0)
        total = float(cycles.sum())
        print("with stamps: %.2f ms" % stamped)
        print("section          share of wave cycles")
        for name, c in zip(SECTIONS, cycles):
            print("%-16s %6.3f" % (name, float(c) / total))
        # block end times, 100 MHz ticks -> ms since the launch's start
        t = (ends.astype(np.int64) - start) * 1e-5
        t = t[ends != 0]
        last = t.max()
        print("blocks: %d; the launch ends %.2f ms after its first block "
              "started" % (len(t), last))
        print("a block's end before the launch's end, ms: "
              "median %.2f  p10 %.2f  p90 %.2f  earliest %.2f"
              % (np.median(last - t), np.percentile(last - t, 10),
                 np.percentile(last - t, 90), (last - t).max()))
        # what the blocks that have left leave idle: wave slots x time
        print("idle share of the launch's block-time after blocks left: %.3f"
              % (float((last - t).sum()) / (len(t) * last)))
        for q in (0.5, 0.25, 0.1, 0.05):
            # when only a fraction q of the blocks is still running
            print("  %4.0f %% of the blocks still run %.2f ms before the end"
                  % (100 * q, last - np.quantile(t, 1 - q)))
        eng.close()
    if len(points) >= 2:
        x = np.array([p[0] for p in points])
        y = np.array([p[1] for p in points])
        slope, intercept = np.polyfit(x, y, 1)
        print("kernel time = %.3f ms + %.4f ms per step per packet "
              "(least squares over %d grids)" % (intercept, slope, len(x)))


if __name__ == "__main__":
    main()
