#!/usr/bin/env python3
"""Host-side count for the padded march's block table: how many of the cells
a ray bundle crosses find their first slot taken by ANOTHER cell of the same
bundle (they chain: a second probe, or after CMI_TABLE_PROBES a global
atomic).

A bundle is 64 rays from one point into one direction bin of the sort (21
bits: 2.4e-3 rad across), through a padded grid of 258^3 cells; its cells
are the padded long indices of points sampled along the rays. Two hashes of the record's byte
offset (8 x the padded index), for tables of 2048 and 4096 slots:

    low   the kernel's: v_mul_u32_u24 by 0x9e3779, the TOP bits of the low 24
          bits of the product (Fibonacci hashing modulo 2^24)
    high  v_mul_hi_u32_u24 by a 24-bit constant, slot bits taken from the
          product's bits 32 and up (so that one v_and_b32 gives the tag's
          byte address)

    python tools/pad_hash_chains.py
"""
import numpy as np

N = 258
K = 0x9e3779


def bundle_cells(origin, direction, rng):
    d = direction / np.linalg.norm(direction)
    rays = d + 2.4e-3 * rng.uniform(-0.5, 0.5, size=(64, 3))
    rays /= np.linalg.norm(rays, axis=1)[:, None]
    t = np.arange(0., 2. * N, 0.25)
    pts = origin + t[:, None, None] * rays[None]
    idx = np.floor(pts).astype(np.int64)
    ok = np.all((idx >= 1) & (idx < N - 1), axis=2)
    cells = (idx[..., 0] * N + idx[..., 1]) * N + idx[..., 2]
    return np.unique(cells[ok])


def slots(cells, bits, kind, k=K):
    offset = (cells << 3) & 0xffffff          # the multiply's 24 bits
    product = offset * k
    if kind == "low":
        return (product >> (24 - bits + 3)) & ((1 << bits) - 1)
    # bits [34, 34 + bits) of the product: (hi & mask << 2) is 4 x the slot
    return (product >> 34) & ((1 << bits) - 1)


def chained(s):
    """cells whose slot another cell of the bundle has too"""
    _, counts = np.unique(s, return_counts=True)
    return int((counts - 1).sum())


def main():
    rng = np.random.default_rng(1)
    origin = np.array([129.3, 128.6, 129.4])
    directions = [(1., 0.03, 0.02), (0.02, 1., 0.03), (0.03, 0.02, 1.),
                  (1., 1., 0.05), (1., 0.05, 1.), (1., 1., 1.),
                  (-0.3, 0.8, 0.52), (0.61, -0.2, -0.77)]
    print("%-22s %6s | %-11s | %-11s" % ("direction", "cells", "2048 slots",
                                         "4096 slots"))
    print("%-22s %6s | %5s %5s | %5s %5s" % ("", "", "low", "high", "low",
                                             "high"))
    for d in directions:
        cells = bundle_cells(origin, np.array(d), rng)
        row = [chained(slots(cells, b, kind)) for b in (11, 12)
               for kind in ("low", "high")]
        print("%-22s %6d | %5d %5d | %5d %5d" % ((str(d), cells.size) +
                                                 tuple(row)))


if __name__ == "__main__":
    main()
