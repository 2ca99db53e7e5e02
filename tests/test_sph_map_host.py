"""The host side of the SPH mappings (cmacionize_amd/csrc/sph_map_plan.h):
the tiles and candidate cells of a particle's reach box, the list sizes, the
class split and the decline rules, called from a small stand-alone program and
checked against plain numpy; and the brute force of tests/sph_map_lib.py - the
yardstick of the GPU tests - against the host's own "centroid" mapping, which
the reference's known answers pin."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import sph_map_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "cmacionize_amd", "csrc")
LIB = os.path.join(ROOT, "cmacionize_amd", "libcmi_gpu_library.so")
M_H = 1.6737236e-27
TILE = (4, 8, 8)
LANE_CANDIDATES = 64

PROGRAM = r"""
#include "sph_map_plan.h"
#include <cstdio>
int main() {
  char what;
  SphMapGeometry g = {};
  int form = 0;
  while (std::scanf(" %c", &what) == 1) {
    if (what == 'G') {
      double anchor[3], sides[3], box[3];
      int32_t ncell[3];
      int periodic;
      if (std::scanf("%la %la %la %la %la %la %d %d %d %d %la %la %la %d",
                     anchor, anchor + 1, anchor + 2, sides, sides + 1,
                     sides + 2, ncell, ncell + 1, ncell + 2, &periodic, box,
                     box + 1, box + 2, &form) != 14)
        return 1;
      g = cmi_sph_geometry(anchor, sides, ncell, periodic ? box : nullptr);
      std::printf("%d %d %d %d %d %d %d\n", g.ntile[0], g.ntile[1],
                  g.ntile[2], CMI_SPH_TILE_X, CMI_SPH_TILE_Y, CMI_SPH_TILE_Z,
                  CMI_SPH_LANE_CANDIDATES);
    } else if (what == 'P') {
      double p[3], h;
      if (std::scanf("%la %la %la %la", p, p + 1, p + 2, &h) != 4)
        return 1;
      SphTileRange r;
      const double reach = cmi_sph_reach(form, h);
      const long long tiles = cmi_sph_particle_tiles(g, p, reach, r);
      const long long candidates = cmi_sph_particle_candidates(g, p, reach);
      std::printf("%lld %lld %d", tiles, candidates,
                  cmi_sph_particle_class(candidates));
      for (int a = 0; a < 3; ++a) {
        std::printf(" %d", r.n[a]);
        for (int k = 0; k < 3; ++k)
          std::printf(" %d %d", k < r.n[a] ? r.lo[a][k] : 0,
                      k < r.n[a] ? r.hi[a][k] : -1);
      }
      std::printf("\n");
    } else if (what == 'D') {
      long long n, entries, cap;
      double largest, box[3];
      int periodic;
      if (std::scanf("%lld %la %d %la %la %la %lld %lld", &n, &largest,
                     &periodic, box, box + 1, box + 2, &entries, &cap) != 8)
        return 1;
      std::printf("%d %d %lld\n",
                  cmi_sph_decline_early(n, largest, periodic ? box : nullptr),
                  cmi_sph_decline_lists(entries, cap),
                  (long long)CMI_SPH_LIST_CAP);
    } else {
      return 1;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = (os.environ.get("CXX") or shutil.which("c++") or
           shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no C++ compiler for the stand-alone planner program"
    d = tmp_path_factory.mktemp("sph_map_plan")
    src = d / "plan.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I", HEADER_DIR, "-o", str(exe), str(src)], check=True)

    def run(text):
        out = subprocess.run([str(exe)], input=text, capture_output=True,
                             text=True, check=True).stdout
        return [[int(x) for x in line.split()] for line in out.splitlines()]
    return run


def hexes(values):
    return " ".join(float(v).hex() for v in values)


def plan_of(planner, case, form):
    """the program's answer for every particle of a case"""
    anchor, sides, ncell = case["grid"]
    box = case["periodic_box"]
    text = "G %s %s %d %d %d %d %s %d\n" % (
        hexes(anchor), hexes(sides), ncell[0], ncell[1], ncell[2],
        0 if box is None else 1, hexes(np.zeros(3) if box is None
                                       else box[3:]), form)
    for p, h in zip(case["positions"], case["h"]):
        text += "P %s %s\n" % (hexes(p), float(h).hex())
    out = planner(text)
    ntile = tuple(out[0][:3])
    assert tuple(out[0][3:6]) == TILE and out[0][6] == LANE_CANDIDATES
    assert ntile == tuple(-(-ncell[a] // TILE[a]) for a in range(3))
    rows = np.array(out[1:], dtype=np.int64)
    assert len(rows) == len(case["h"])
    # per particle and axis: which tiles its intervals hold
    masks = []
    for a in range(3):
        mask = np.zeros((len(rows), ntile[a]), dtype=bool)
        base = 3 + 7 * a
        for k in range(3):
            lo, hi = rows[:, base + 1 + 2 * k], rows[:, base + 2 + 2 * k]
            used = k < rows[:, base]
            t = np.arange(ntile[a])[None, :]
            mask |= used[:, None] & (t >= lo[:, None]) & (t <= hi[:, None])
        # intervals are disjoint: their lengths add up to the mask
        length = sum(np.where(k < rows[:, base],
                              rows[:, base + 2 + 2 * k] -
                              rows[:, base + 1 + 2 * k] + 1, 0)
                     for k in range(3))
        assert np.array_equal(length, mask.sum(axis=1))
        masks.append(mask)
    return dict(tiles=rows[:, 0], candidates=rows[:, 1], cls=rows[:, 2],
                masks=masks, ntile=ntile)


def reach_box_cells(case, form):
    """numpy, per axis: the cells whose midpoint lies in the reach box of a
    particle or of one of its two periodic images (n, ncell[a]) booleans"""
    anchor, sides, ncell = case["grid"]
    box = case["periodic_box"]
    reach = S.reach_of(form, case["h"])
    out = []
    for a in range(3):
        side = sides[a] / ncell[a]
        mid = (anchor[a] + side * np.arange(ncell[a])) + 0.5 * side
        hit = np.zeros((len(reach), ncell[a]), dtype=bool)
        for s in ((-1, 0, 1) if box is not None else (0,)):
            q = case["positions"][:, a] + (s * box[3 + a] if s else 0.)
            hit |= np.abs(mid[None, :] - q[:, None]) <= reach[:, None]
        out.append(hit)
    return out


@functools.lru_cache(maxsize=None)
def cached_case(name):
    return {"A": lambda: S.case_a(False), "B": lambda: S.case_a(True),
            "C": S.case_c}[name]()


@functools.lru_cache(maxsize=None)
def cached_pairs(name, form):
    c = cached_case(name)
    return S.Pairs(c["positions"], c["h"], form, c["grid"], c["periodic_box"])


@pytest.mark.parametrize("name,form", [("A", 0), ("A", 1), ("B", 0), ("B", 1),
                                       ("C", 0)])
def test_tile_ranges_cover_every_pair_and_lists_match(planner, name, form):
    case = cached_case(name)
    ncell = case["grid"][2]
    plan = plan_of(planner, case, form)
    pairs = cached_pairs(name, form)
    assert len(pairs.i) > 1000
    # every contributing pair's cell lies in a tile of its particle's range
    cz = pairs.c % ncell[2]
    cy = (pairs.c // ncell[2]) % ncell[1]
    cx = pairs.c // (ncell[2] * ncell[1])
    for a, cell in enumerate((cx, cy, cz)):
        assert plan["masks"][a][pairs.i, cell // TILE[a]].all(), \
            "axis %d: a pair within reach whose tile is not listed" % a
    # the lists: per tile, the particles whose reach box touches it
    hits = reach_box_cells(case, form)
    tile_hits = []
    for a in range(3):
        t = np.zeros((len(case["h"]), plan["ntile"][a]), dtype=bool)
        for cell in range(ncell[a]):
            t[:, cell // TILE[a]] |= hits[a][:, cell]
        tile_hits.append(t)
        assert np.array_equal(t, plan["masks"][a]), "axis %d" % a
    brute = np.einsum("ia,ib,ic->abc", *[t.astype(np.int64)
                                         for t in tile_hits])
    planned = np.einsum("ia,ib,ic->abc", *[m.astype(np.int64)
                                           for m in plan["masks"]])
    assert np.array_equal(brute, planned)
    assert plan["tiles"].sum() == brute.sum()
    assert np.array_equal(plan["tiles"], np.prod(
        [t.sum(axis=1) for t in tile_hits], axis=0))
    if name == "B":
        # kernels do cross the periodic faces: along every axis some reach
        # box holds the first and the last cell and not all between
        for a in range(3):
            crosses = hits[a][:, 0] & hits[a][:, -1] & ~hits[a].all(axis=1)
            assert crosses.sum() >= 5
        corner = np.all([h[:, 0] & h[:, -1] & ~h.all(axis=1) for h in hits],
                        axis=0)
        assert corner.any()
    if name == "A":
        # particles far outside touch nothing; some outside reach in
        outside = np.any((case["positions"] < case["grid"][0]) |
                         (case["positions"] > case["grid"][0] +
                          case["grid"][1]), axis=1)
        assert (plan["tiles"][outside] == 0).sum() >= 20
        assert (plan["tiles"][outside] > 0).sum() >= 20


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_class_split_follows_the_candidate_count(planner, name):
    case = cached_case(name)
    for form in (0, 1):
        plan = plan_of(planner, case, form)
        count = np.prod([h.sum(axis=1) for h in reach_box_cells(case, form)],
                        axis=0)
        assert np.array_equal(plan["candidates"], count)
        expect = np.where(count == 0, 0,
                          np.where(count <= LANE_CANDIDATES, 1, 2))
        assert np.array_equal(plan["cls"], expect)
        # every pair within reach is a candidate of its particle
        if name != "C" or form == 0:
            pairs = cached_pairs(name, form)
            assert np.all(np.bincount(pairs.i, minlength=len(count)) <= count)
    # (the periodic case caps h: only the wider form has a wave class there)
    plan = plan_of(planner, case, 1 if name == "B" else 0)
    assert (plan["cls"] == 1).any() and (plan["cls"] == 2).any()
    if name == "C":
        near = np.abs(plan["candidates"] - LANE_CANDIDATES) <= 40
        assert (plan["cls"][near] == 1).any() and (plan["cls"][near] == 2).any()


def test_decline_rules(planner):
    def ask(n, largest, box, entries, cap):
        text = "D %d %s %d %s %d %d\n" % (
            n, float(largest).hex(), 0 if box is None else 1,
            hexes(np.zeros(3) if box is None else box), entries, cap)
        return planner(text)[0]
    box = (3., 2., 5.)
    assert ask(10, 0.9, box, 5, 10)[:2] == [0, 0]
    assert ask(0, 0.9, box, 0, 10)[0] == 1                 # no particles
    assert ask(10, 1.0, box, 5, 10)[0] == 2                # 2 reach = L
    assert ask(10, 1.5, box, 5, 10)[0] == 2                # 2 reach > L
    assert ask(10, np.nextafter(1., 0.), box, 5, 10)[0] == 0
    assert ask(10, 100., None, 5, 10)[0] == 0              # no box, no wrap
    assert ask(10, 0.1, box, 11, 10)[1] == 3               # lists over the cap
    assert ask(10, 0.1, box, 10, 10)[1] == 0
    assert ask(10, 0.1, box, 1, 1)[2] == 1 << 28           # the engine's cap


def test_brute_force_reproduces_the_host_centroid_mapping():
    """cmi_gpu_library_map_to_cells(b"centroid") on case A: density / m_H
    where a kernel covers the midpoint, the floor m[0] / V 1e-6 elsewhere."""
    assert os.path.exists(LIB), "build() makes libcmi_gpu_library.so"
    L = C.CDLL(LIB)
    vp = C.c_void_p
    L.cmi_gpu_library_map_to_cells.argtypes = [
        C.c_char_p, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, C.c_double,
        C.c_double, vp, vp, vp, vp, vp]
    case = cached_case("A")
    anchor, sides, ncell = case["grid"]
    x, y, z = (np.ascontiguousarray(case["positions"][:, a])
               for a in range(3))
    h = np.ascontiguousarray(case["h"])
    m = np.ascontiguousarray(case["amplitudes"][0])
    nc = np.array(ncell, dtype=np.int32)
    host = np.zeros(int(np.prod(ncell)))
    rc = L.cmi_gpu_library_map_to_cells(
        b"centroid", 0, x.ctypes.data, y.ctypes.data, z.ctypes.data,
        h.ctypes.data, m.ctypes.data, len(h), 1., 1., None,
        np.ascontiguousarray(anchor).ctypes.data,
        np.ascontiguousarray(sides).ctypes.data, nc.ctypes.data,
        host.ctypes.data)
    assert rc == 0
    expect, tol = cached_pairs("A", 0).to_cells(m)
    expect, tol = expect[0], tol[0]
    empty = tol == 0.
    assert empty.any() and not empty.all()
    volume = np.prod(sides / np.array(ncell))
    assert np.all(host[empty] == m[0] / volume * 1.e-6 / M_H)
    err = np.abs(host - expect / M_H)[~empty]
    print("host centroid against the brute force: worst error / bound = %.3g"
          % np.max(err / (tol[~empty] / M_H)))
    assert np.all(err <= tol[~empty] / M_H)
