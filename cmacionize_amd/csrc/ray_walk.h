/*
 * ray_walk.h - the geometry of the ray-traced renderers (line and sky images,
 * line and sky cubes, continuum images, absorbing cubes), stated once: how a
 * ray of either camera enters the grid and walks it cell by cell (GridRay),
 * which sample ray a thread of the parallel camera has (tile_sample), the
 * velocity edges of a block of channels (channel_block_edges) and the rows of
 * the probes (probe_row). Nothing of the physics: what a renderer does with a
 * cell and its path length stands in its own kernel.
 *
 * Parallel camera (view angles theta, phi; all of it computed once on the
 * host and passed by value, LineViewDev):
 *   n   = (sin theta cos phi, sin theta sin phi, cos theta)  to the observer
 *   e_x = (-sin phi, cos phi, 0)
 *   e_y = (-cos theta cos phi, -cos theta sin phi, sin theta)
 * Sample (a, b) of pixel (ix, iy) at supersampling s has image coordinates
 *   x = anchor[0] + sides[0] * ((ix + (a + 0.5) / s) / nx),  y likewise,
 * its ray is o + t n with o = x e_x + y e_y, clipped to the box by a slab
 * test: per axis with n != 0, t0 = (lo - o) / n, t1 = (hi - o) / n (as
 * products with 1 / n), t_in = max over axes of min(t0, t1), t_out = min of
 * max(t0, t1); an axis with n == 0 only asks lo <= o < hi. A ray hits if
 * t_in < t_out and both are finite (a NaN coordinate passes through fmax and
 * fmin and leaves them infinite: such a ray misses, it must never reach the
 * march, whose NaN step would advance no index). It starts at o + t_in n,
 * in the cell floor() of that point gives, clamped into the grid.
 *
 * Point camera: ray r is o + t d_r, t >= 0; d_r is used as given (the host
 * has checked | |d|^2 - 1 | <= 1e-9 and that everything is finite), 1 / d is
 * the lane's own division. The slab test is the same with the lane's 1 / d.
 * t_start = t_in if t_in > 0, else 0; the ray hits if t_start < t_out and
 * t_out is finite. With t_in <= 0 (the origin is in the box) the march starts
 * at o itself, otherwise at o + t_in d; in either case in the cell
 * floor((p - anchor) inv_cellside) gives, clamped into the grid. An origin on
 * a cell wall with a direction pointing back across it makes a first step of
 * length 0; nothing treats it specially.
 *
 * The step is the EXACT marcher's arithmetic (dda_step<false> of
 * device_transport.h at tau = HUGE_VAL: the walls of the cell from its index,
 * the wall distances from the current position, every tying axis advances,
 * DBL_MAX for a zero direction component). GridRay::step restates those
 * operations one for one rather than calling dda_step, which loads a 16-B
 * transport record per cell; here the record is the renderer's. The march
 * ends when the index leaves the grid (at least one component of a unit
 * vector is normal, so at least one index moves at every step).
 *
 * Mapping of the parallel camera: one lane per sample ray; a wave is an 8 x 8
 * tile of the sample grid (nx s) x (ny s) and a workgroup of four waves a
 * 16 x 16 tile, so that the rays of a wave form a bundle that crosses the
 * same few cache lines of records at every step (DESIGN.md 4.7 has what was
 * measured and what was not).
 */
#ifndef CMI_RAY_WALK_H
#define CMI_RAY_WALK_H

#include "device_common.h"

#ifndef CMI_LINE_IMAGE_TILE_X
#define CMI_LINE_IMAGE_TILE_X 8 /* wave tile: TILE_X x (64 / TILE_X) samples */
#endif

struct LineViewDev {
  double n[3], inv_n[3], ex[3], ey[3];
  double img_anchor[2], img_sides[2];
  int32_t nx, ny, s;
  int32_t pad;
};

/* a lane's ray: the direction and its inverse, where it is and in which cell,
 * and the parameters at which it enters (t0: t_in of the parallel camera,
 * t_start of the point camera) and leaves (t1) the box */
struct GridRay {
  double d[3], inv_d[3], pos[3];
  int32_t index[3];
  double t0, t1;

  /* axis a of the slab test of o + t d, o_a = o[a]: narrows (t_in, t1), or,
   * without a direction component, asks whether o_a is inside */
  __device__ __forceinline__ void slab(const GridDev &g, int a, double o_a,
                                       double &t_in, bool &hit) {
    const double lo = g.anchor[a];
    const double hi = g.anchor[a] + g.box_sides[a];
    if (d[a] != 0.) {
      const double ta = (lo - o_a) * inv_d[a];
      const double tb = (hi - o_a) * inv_d[a];
      t_in = fmax(t_in, fmin(ta, tb));
      t1 = fmin(t1, fmax(ta, tb));
    } else {
      hit = hit && (o_a >= lo && o_a < hi);
    }
  }

  /* the cell of pos, clamped: an origin on the upper face, or an entry point
   * that rounding put a hair outside the box */
  __device__ __forceinline__ void enter(const GridDev &g) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double c = floor((pos[a] - g.anchor[a]) * g.inv_cellside[a]);
      c = fmin(fmax(c, 0.), (double)(g.ncell[a] - 1));
      index[a] = (int32_t)c;
    }
  }

  /* the ray of image coordinates (x, y) of the parallel camera: false if it
   * misses the box (t0 and t1 are then whatever the slab test left);
   * otherwise at the entry point, in the cell the march starts in */
  __device__ __forceinline__ bool start(const GridDev &g, const LineViewDev &v,
                                        double x, double y) {
    double o[3];
    bool hit = true;
    t0 = -HUGE_VAL;
    t1 = HUGE_VAL;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      d[a] = v.n[a];
      inv_d[a] = v.inv_n[a];
      o[a] = x * v.ex[a] + y * v.ey[a];
      slab(g, a, o[a], t0, hit);
    }
    hit = hit && (t0 < t1) && t0 > -HUGE_VAL && t1 < HUGE_VAL;
    if (!hit)
      return false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      pos[a] = o[a] + t0 * d[a];
    enter(g);
    return true;
  }

  /* ray r of the point camera at o: false if it misses the box; otherwise at
   * the point, in the cell the march starts in */
  __device__ __forceinline__ bool start(const GridDev &g, const double o[3],
                                        const double *directions, int64_t r) {
    double t_in = -HUGE_VAL;
    bool hit = true;
    t1 = HUGE_VAL;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      d[a] = directions[3 * r + a];
      inv_d[a] = 1. / d[a];
      slab(g, a, o[a], t_in, hit);
    }
    t0 = (t_in > 0.) ? t_in : 0.;
    hit = hit && (t0 < t1) && t1 < HUGE_VAL;
    if (!hit)
      return false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      pos[a] = (t_in > 0.) ? o[a] + t_in * d[a] : o[a];
    enter(g);
    return true;
  }

  __device__ __forceinline__ bool inside(const GridDev &g) const {
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      in &= (index[a] >= 0 && index[a] < g.ncell[a]);
    return in;
  }

  __device__ __forceinline__ int64_t cell(const GridDev &g) const {
    return ((int64_t)index[0] * g.ncell[1] + index[1]) * g.ncell[2] + index[2];
  }

  /* the geometry of dda_step<false> (device_transport.h) at tau = HUGE_VAL,
   * the same operations in the same order: returns the path length in the
   * cell, moves pos to the wall and index across it */
  __device__ __forceinline__ double step(const GridDev &g) {
    double w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double lo = g.anchor[a] + g.cellside[a] * (index[a] + g.offset[a]);
      const double hi = lo + g.cellside[a];
      w[a] = (d[a] > 0.) ? (hi - pos[a]) * inv_d[a]
                         : ((d[a] < 0.) ? (lo - pos[a]) * inv_d[a] : DBL_MAX);
    }
    const double ds = fmin(w[0], fmin(w[1], w[2]));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      /* every axis that ties the minimum advances (edges, corners) */
      const int32_t across = (w[a] == ds) ? ((d[a] > 0.) ? 1 : -1) : 0;
      pos[a] = pos[a] + ds * d[a];
      index[a] += across;
    }
    return ds;
  }
};

/* ---- the parallel camera's threads: a workgroup is 2 x 2 wave tiles ---- */

/* workgroups of a chunk of nsx sample columns by NY sample rows */
inline unsigned tile_workgroups(int64_t nsx, int64_t NY) {
  constexpr int TX = CMI_LINE_IMAGE_TILE_X, TY = 64 / TX;
  const int64_t tiles_y = (NY + 2 * TY - 1) / (2 * TY);
  const int64_t tiles_x = (nsx + 2 * TX - 1) / (2 * TX);
  return (unsigned)(tiles_x * tiles_y);
}

/* the thread's sample (sx, sy) of the chunk's columns [sx0, sx1) and its
 * image coordinates; false if the thread has none */
__device__ __forceinline__ bool tile_sample(const LineViewDev &v, int32_t sx0,
                                            int32_t sx1, int32_t &sx,
                                            int32_t &sy, double &x,
                                            double &y) {
  constexpr int TX = CMI_LINE_IMAGE_TILE_X, TY = 64 / TX;
  const int32_t NY = v.ny * v.s;
  const int32_t tiles_y = (NY + 2 * TY - 1) / (2 * TY);
  const int32_t by = blockIdx.x % tiles_y, bx = blockIdx.x / tiles_y;
  const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  sx = sx0 + (2 * bx + (wave >> 1)) * TX + lane / TY;
  sy = (2 * by + (wave & 1)) * TY + lane % TY;
  if (sx >= sx1 || sy >= NY)
    return false;
  const int32_t ix = sx / v.s, iy = sy / v.s;
  const double fa = ((sx - ix * v.s) + 0.5) / v.s;
  const double fb = ((sy - iy * v.s) + 0.5) / v.s;
  x = v.img_anchor[0] + v.img_sides[0] * ((ix + fa) / v.nx);
  y = v.img_anchor[1] + v.img_sides[1] * ((iy + fb) / v.ny);
  return true;
}

/* where a plane of the chunk's samples holds sample (sx, sy) */
__device__ __forceinline__ int64_t tile_sample_at(const LineViewDev &v,
                                                  int32_t sx0, int32_t sx,
                                                  int32_t sy) {
  return (int64_t)(sx - sx0) * (v.ny * v.s) + sy;
}

/* ---- a block of CB consecutive velocity channels [c0, c0 + nc) ---- */

/* the block's edges e_c = vmin + c dv; those past the last channel of a
 * partial block repeat its upper edge (their channels are empty and not
 * stored) */
template <int CB>
__device__ __forceinline__ void channel_block_edges(double vmin, double dv,
                                                    int32_t c0, int32_t nc,
                                                    double edge[CB + 1]) {
#pragma unroll
  for (int i = 0; i <= CB; ++i)
    edge[i] = vmin + (double)(c0 + (i < nc ? i : nc)) * dv;
}

/* z of the block's lowest and highest edge: every edge at or below -6 (or
 * NaN: b == 0 and u on the upper edge), or every edge at or above 6, so that
 * f_c == 0 for the whole block */
__device__ __forceinline__ bool channel_block_dark(double z_lo, double z_hi) {
  return !(z_hi > -6.) || (z_lo >= 6.);
}

/* ---- the probes ---- */

/* the row prefix {t0, t1, steps, cells[max_cells], ds[max_cells]} of a ray
 * after its start() (hit: what that returned), {NaN, NaN, 0} for a miss:
 * walks the ray to the end; per_step(cell, ds, step) is what the probe does
 * in a cell, after the step out of it */
template <class F>
__device__ __forceinline__ void probe_row(const GridDev &g, GridRay &ray,
                                          bool hit, int32_t max_cells,
                                          double *o, F per_step) {
  int steps = 0;
  if (hit) {
    while (ray.inside(g)) {
      const int64_t cell = ray.cell(g);
      const double ds = ray.step(g);
      per_step(cell, ds, steps);
      if (steps < max_cells) {
        o[3 + steps] = (double)cell;
        o[3 + max_cells + steps] = ds;
      }
      ++steps;
    }
  }
  o[0] = hit ? ray.t0 : __builtin_nan("");
  o[1] = hit ? ray.t1 : __builtin_nan("");
  o[2] = (double)steps;
}

#endif
