/*
 * sph_map_plan.h - the arithmetic both SPH mappings (sph_map_kernels.h) are
 * planned with: the tiles the grid is cut into, the cells and tiles a
 * particle's reach box touches (also across the faces of a periodic box), the
 * class a particle is gathered in, and when a call declines. Plain C++ with no
 * device code of its own: the kernels call the same functions as the host,
 * and a stand-alone program can call them (tests/test_sph_map_host.py).
 *
 * A cell index is z-fastest; the midpoint of cell i along an axis is
 * (anchor + side * i) + 0.5 * side with side = sides / ncell, the same
 * sequence of operations as the host grid's.
 */
#ifndef CMI_SPH_MAP_PLAN_H
#define CMI_SPH_MAP_PLAN_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CMI_SPH_HD __host__ __device__
#else
#define CMI_SPH_HD
#endif

/* kernel forms: 0 the cubic spline with support h (CubicSplineKernel), 1 the
 * M4 spline of Price 2007 with support 2 h */
#define CMI_SPH_FORM_SPLINE_H 0
#define CMI_SPH_FORM_SPLINE_2H 1

/* a tile is 4 x 8 x 8 cells (x, y, z): 256 cells, one lane each, a wave is
 * one x-layer of 8 rows of 8 cells that lie together in memory */
#define CMI_SPH_TILE_X 4
#define CMI_SPH_TILE_Y 8
#define CMI_SPH_TILE_Z 8
#define CMI_SPH_TILE_CELLS 256
/* particle records a workgroup stages through LDS at a time */
#define CMI_SPH_STAGE_CHUNK 128
/* most amplitude arrays of one call */
#define CMI_SPH_MAX_AMPLITUDES 4
/* most candidate midpoints of a particle that one lane gathers; above, a
 * wave does */
#define CMI_SPH_LANE_CANDIDATES 64
/* most (tile, particle) list entries of a call, 4 bytes each: 1 GiB */
#define CMI_SPH_LIST_CAP ((int64_t)1 << 28)
/* the reach box is widened by this fraction of a cell side, so that the
 * rounding of the index arithmetic cannot drop a midpoint within reach */
#define CMI_SPH_INDEX_SLACK 1.e-9

/* why a call declined (cmi_gpu_get_sph_map_stats) */
enum {
  CMI_SPH_TAKEN = 0,
  CMI_SPH_DECLINE_NO_PARTICLES = 1,
  CMI_SPH_DECLINE_WIDE_KERNEL = 2,
  CMI_SPH_DECLINE_LIST_SIZE = 3
};

struct SphMapGeometry {
  double anchor[3], side[3]; /* of the grid; side of a CELL */
  int32_t ncell[3];
  int32_t ntile[3];
  int32_t periodic; /* a periodic box is set */
  double box[3];    /* its sides */
};

static inline CMI_SPH_HD int cmi_sph_tile_dim(int a) {
  return a == 0 ? CMI_SPH_TILE_X : (a == 1 ? CMI_SPH_TILE_Y : CMI_SPH_TILE_Z);
}

static inline SphMapGeometry cmi_sph_geometry(const double *anchor,
                                              const double *sides,
                                              const int32_t *ncell,
                                              const double *periodic_sides) {
  SphMapGeometry g = {};
  for (int a = 0; a < 3; ++a) {
    g.anchor[a] = anchor[a];
    g.side[a] = sides[a] / ncell[a];
    g.ncell[a] = ncell[a];
    g.ntile[a] = (ncell[a] + cmi_sph_tile_dim(a) - 1) / cmi_sph_tile_dim(a);
    g.box[a] = periodic_sides ? periodic_sides[a] : 0.;
  }
  g.periodic = periodic_sides ? 1 : 0;
  return g;
}

static inline CMI_SPH_HD double cmi_sph_midpoint(const SphMapGeometry &g, int a,
                                                 int32_t i) {
  return (g.anchor[a] + g.side[a] * i) + 0.5 * g.side[a];
}

static inline CMI_SPH_HD double cmi_sph_reach(int form, double h) {
  return form == CMI_SPH_FORM_SPLINE_2H ? 2. * h : h;
}

/* The separation the kernel sums use along one axis: the minimum image of
 * Box::periodic_distance in a periodic box, applied once. */
static inline CMI_SPH_HD double cmi_sph_separation(const SphMapGeometry &g,
                                                   int a, double c, double p) {
  double d = c - p;
  if (g.periodic) {
    if (2. * d < -g.box[a])
      d += g.box[a];
    if (2. * d >= g.box[a])
      d -= g.box[a];
  }
  return d;
}

/* The cells along axis a whose midpoint can lie within `reach` of a particle
 * at p: up to three ascending, disjoint, inclusive index intervals - one per
 * image of the particle in a periodic box, which cannot overlap while
 * 2 reach < box side -, clipped to the grid. Returns their number. */
static inline CMI_SPH_HD int cmi_sph_axis_cells(const SphMapGeometry &g, int a,
                                                double p, double reach,
                                                int32_t lo[3], int32_t hi[3]) {
  int n = 0;
  const int first = g.periodic ? -1 : 0, last = g.periodic ? 1 : 0;
  for (int s = first; s <= last; ++s) {
    const double q = p + s * g.box[a];
    const double from =
        (q - reach - g.anchor[a]) / g.side[a] - 0.5 - CMI_SPH_INDEX_SLACK;
    const double to =
        (q + reach - g.anchor[a]) / g.side[a] - 0.5 + CMI_SPH_INDEX_SLACK;
    if (!(to >= 0.) || !(from <= (double)(g.ncell[a] - 1)))
      continue; /* (also: not a number) */
    int32_t l = from <= 0. ? 0 : (int32_t)ceil(from);
    int32_t h = to >= (double)(g.ncell[a] - 1) ? g.ncell[a] - 1
                                                : (int32_t)floor(to);
    /* (the slack may make neighbouring images meet) */
    if (n > 0 && l <= hi[n - 1])
      l = hi[n - 1] + 1;
    if (l > h)
      continue;
    lo[n] = l;
    hi[n] = h;
    ++n;
  }
  return n;
}

/* ... and the tiles those cells lie in: ascending, disjoint intervals */
static inline CMI_SPH_HD int cmi_sph_axis_tiles(const SphMapGeometry &g, int a,
                                                double p, double reach,
                                                int32_t lo[3], int32_t hi[3]) {
  int32_t clo[3], chi[3];
  const int nc = cmi_sph_axis_cells(g, a, p, reach, clo, chi);
  const int dim = cmi_sph_tile_dim(a);
  int n = 0;
  for (int k = 0; k < nc; ++k) {
    int32_t l = clo[k] / dim;
    const int32_t h = chi[k] / dim;
    if (n > 0 && l <= hi[n - 1])
      l = hi[n - 1] + 1; /* two images in one tile: listed once */
    if (l > h)
      continue;
    lo[n] = l;
    hi[n] = h;
    ++n;
  }
  return n;
}

static inline CMI_SPH_HD int64_t cmi_sph_interval_cells(int n,
                                                        const int32_t lo[3],
                                                        const int32_t hi[3]) {
  int64_t c = 0;
  for (int k = 0; k < n; ++k)
    c += hi[k] - lo[k] + 1;
  return c;
}

/* The particle's tiles: per axis the intervals above. Returns how many tiles
 * that is (the particle's list entries). */
struct SphTileRange {
  int32_t n[3], lo[3][3], hi[3][3];
};
static inline CMI_SPH_HD int64_t cmi_sph_particle_tiles(const SphMapGeometry &g,
                                                        const double p[3],
                                                        double reach,
                                                        SphTileRange &r) {
  int64_t count = 1;
  for (int a = 0; a < 3; ++a) {
    r.n[a] = cmi_sph_axis_tiles(g, a, p[a], reach, r.lo[a], r.hi[a]);
    count *= cmi_sph_interval_cells(r.n[a], r.lo[a], r.hi[a]);
  }
  return count;
}

/* The candidate midpoints of a particle: the cells of its reach box. */
static inline CMI_SPH_HD int64_t cmi_sph_particle_candidates(
    const SphMapGeometry &g, const double p[3], double reach) {
  int64_t count = 1;
  for (int a = 0; a < 3; ++a) {
    int32_t lo[3], hi[3];
    const int n = cmi_sph_axis_cells(g, a, p[a], reach, lo, hi);
    count *= cmi_sph_interval_cells(n, lo, hi);
  }
  return count;
}

/* 0: no candidate, the particle's sum is 0; 1: one lane gathers it; 2: a wave */
static inline CMI_SPH_HD int cmi_sph_particle_class(int64_t candidates) {
  return candidates <= 0 ? 0
                         : (candidates <= CMI_SPH_LANE_CANDIDATES ? 1 : 2);
}

/* Whether a call declines before anything is counted: no particles, or - in
 * a periodic box - a kernel so wide that a cell could see two images of one
 * particle (twice the largest reach not below the smallest side). */
static inline int cmi_sph_decline_early(int64_t n, double largest_reach,
                                        const double *periodic_sides) {
  if (n <= 0)
    return CMI_SPH_DECLINE_NO_PARTICLES;
  if (periodic_sides) {
    double smallest = periodic_sides[0];
    for (int a = 1; a < 3; ++a)
      smallest = periodic_sides[a] < smallest ? periodic_sides[a] : smallest;
    if (!(2. * largest_reach < smallest))
      return CMI_SPH_DECLINE_WIDE_KERNEL;
  }
  return CMI_SPH_TAKEN;
}
/* ... and once the lists are counted */
static inline int cmi_sph_decline_lists(int64_t entries, int64_t cap) {
  return entries > cap ? CMI_SPH_DECLINE_LIST_SIZE : CMI_SPH_TAKEN;
}

#endif /* CMI_SPH_MAP_PLAN_H */
