/*
 * sky_image_kernels.h - sky maps: line images for an observer inside or near
 * the grid. line_image_kernels.h sees the box from infinitely far away, one
 * direction for all rays; here every ray leaves one point, the origin o, in
 * a direction of its own, and the integration runs from the observer
 * outwards, carrying the transmission. The records, the units and the
 * discipline of a CPU restatement (tests/support/sky_image_reference.c) are
 * those of line_image_kernels.h.
 *
 * Geometry: ray r is o + t d_r, t >= 0; d_r is used as given (the host has
 * checked | |d|^2 - 1 | <= 1e-9 and that everything is finite), 1 / d is the
 * lane's own division. The slab test is line_image_ray's with the lane's
 * 1 / d: per axis with d != 0, t0 = (lo - o) (1 / d), t1 = (hi - o) (1 / d),
 * t_in = max over axes of min(t0, t1), t_out = min of max(t0, t1); an axis
 * with d == 0 only asks lo <= o < hi. t_start = t_in if t_in > 0, else 0;
 * the ray hits if t_start < t_out and t_out is finite. With t_in <= 0 (the
 * origin is in the box) the march starts at o itself, otherwise at
 * o + t_in d; in either case in the cell floor((p - anchor) inv_cellside)
 * gives, clamped into the grid. An origin on a cell wall with a direction
 * pointing back across it makes a first step of length 0; nothing treats it
 * specially. The step is line_image_step's - dda_step<false> at tau =
 * HUGE_VAL -, the same operations in the same order with the lane's d and
 * 1 / d: walls from the index, every axis that ties the minimum advances,
 * DBL_MAX for a zero component. The march ends when the index leaves the
 * grid (at least one component of a unit vector is normal, so at least one
 * index moves at every step).
 *
 * Integration, observer outwards: T = 1, I_l = 0; per cell {k, s_0 ..} with
 * path ds
 *   k == 0:  I_l += T * (s_l * ds)
 *   else:    dtau = k * ds;  I_l += T * (s_l * (-expm1(-dtau)));
 *            T = T * exp(-dtau)
 * in exactly this order of multiplications. No atomics: the same call gives
 * the same bits.
 *
 * Mapping: one lane per ray in the caller's order, wave w of a launch takes
 * rays 64 w .. 64 w + 63. Rays of one origin share the cells near it and
 * diverge with distance; the order of the rays is the caller's means to keep
 * a wave's rays together (cmi_gpu_render_line_sky_map orders them in 8 x 8
 * tiles of the map).
 */
#ifndef CMI_SKY_IMAGE_KERNELS_H
#define CMI_SKY_IMAGE_KERNELS_H

#include "line_image_kernels.h"

/* rays per march launch (bounds the direction and result buffers) */
#define CMI_SKY_LAUNCH_RAYS (1ll << 22)

/* a lane's ray: the direction as given and its inverse */
struct SkyRay {
  double d[3], inv_d[3];
};

__device__ __forceinline__ SkyRay sky_load_ray(const double *directions,
                                               int64_t r) {
  SkyRay ray;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ray.d[a] = directions[3 * r + a];
    ray.inv_d[a] = 1. / ray.d[a];
  }
  return ray;
}

/* the ray from o: false if it misses the box (t_start and t_out are then
 * whatever the slab test left); otherwise the point and the cell the march
 * starts in */
__device__ __forceinline__ bool sky_ray_start(const GridDev &g,
                                              const double o[3],
                                              const SkyRay &ray, double pos[3],
                                              int32_t index[3],
                                              double &t_start, double &t_out) {
  double t_in = -HUGE_VAL;
  t_out = HUGE_VAL;
  bool hit = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = g.anchor[a];
    const double hi = g.anchor[a] + g.box_sides[a];
    if (ray.d[a] != 0.) {
      const double t0 = (lo - o[a]) * ray.inv_d[a];
      const double t1 = (hi - o[a]) * ray.inv_d[a];
      t_in = fmax(t_in, fmin(t0, t1));
      t_out = fmin(t_out, fmax(t0, t1));
    } else {
      hit = hit && (o[a] >= lo && o[a] < hi);
    }
  }
  t_start = (t_in > 0.) ? t_in : 0.;
  hit = hit && (t_start < t_out) && t_out < HUGE_VAL;
  if (!hit)
    return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pos[a] = (t_in > 0.) ? o[a] + t_in * ray.d[a] : o[a];
    double c = floor((pos[a] - g.anchor[a]) * g.inv_cellside[a]);
    /* an origin on the upper face, or an entry point that rounding put a
     * hair outside the box */
    c = fmin(fmax(c, 0.), (double)(g.ncell[a] - 1));
    index[a] = (int32_t)c;
  }
  return true;
}

/* line_image_step with the lane's direction: returns the path length in the
 * cell, moves pos to the wall and index across it */
__device__ __forceinline__ double sky_step(const GridDev &g, const SkyRay &ray,
                                           double pos[3], int32_t index[3]) {
  double d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = g.anchor[a] + g.cellside[a] * (index[a] + g.offset[a]);
    const double hi = lo + g.cellside[a];
    d[a] = (ray.d[a] > 0.)
               ? (hi - pos[a]) * ray.inv_d[a]
               : ((ray.d[a] < 0.) ? (lo - pos[a]) * ray.inv_d[a] : DBL_MAX);
  }
  const double ds = fmin(d[0], fmin(d[1], d[2]));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    /* every axis that ties the minimum advances (edges, corners) */
    const int32_t step = (d[a] == ds) ? ((ray.d[a] > 0.) ? 1 : -1) : 0;
    pos[a] = pos[a] + ds * ray.d[a];
    index[a] += step;
  }
  return ds;
}

struct SkyMarchArgs {
  GridDev grid;
  double origin[3];
  const double *directions; /* [nrays][3] */
  const double *records;    /* [ncell][ND] */
  int64_t nrays;
  int32_t nlines; /* lines of the batch: the record's first nlines sources */
  int32_t pad;
  int64_t line_stride; /* ray r of line l goes to out[l * line_stride + r] */
  double *out;
};

/* the march: one lane per ray, observer outwards */
template <int ND>
__global__ void __launch_bounds__(256) sky_march_kernel(const SkyMarchArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrays)
    return;
  const SkyRay ray = sky_load_ray(a.directions, r);

  double I[ND - 1];
#pragma unroll
  for (int l = 0; l < ND - 1; ++l)
    I[l] = 0.;
  double T = 1.;
  double pos[3], t_start, t_out;
  int32_t index[3];
  if (sky_ray_start(a.grid, a.origin, ray, pos, index, t_start, t_out)) {
    while (line_image_inside(a.grid, index)) {
      const int64_t cell =
          ((int64_t)index[0] * a.grid.ncell[1] + index[1]) * a.grid.ncell[2] +
          index[2];
      const double2 *rec =
          reinterpret_cast<const double2 *>(a.records + cell * ND);
      double rc[ND];
#pragma unroll
      for (int h = 0; h < ND / 2; ++h) {
        const double2 w = rec[h];
        rc[2 * h] = w.x;
        rc[2 * h + 1] = w.y;
      }
      const double ds = sky_step(a.grid, ray, pos, index);
      const double k = rc[0];
      if (k == 0.) {
#pragma unroll
        for (int l = 0; l < ND - 1; ++l)
          I[l] += T * (rc[1 + l] * ds);
      } else {
        const double dtau = k * ds;
        const double att = exp(-dtau);
        const double emit = -expm1(-dtau);
#pragma unroll
        for (int l = 0; l < ND - 1; ++l)
          I[l] += T * (rc[1 + l] * emit);
        T = T * att;
      }
    }
  }
  /* (a record of an even number of lines has one padding source) */
#pragma unroll
  for (int l = 0; l < ND - 1; ++l)
    if (l < a.nlines)
      a.out[l * a.line_stride + r] = I[l];
}

/* cmi_gpu_sky_probe: row k = {t_start, t_out, steps, cells[max_cells],
 * ds[max_cells]} of ray k */
__global__ void __launch_bounds__(64)
    sky_probe_kernel(GridDev g, double ox, double oy, double oz,
                     const double *__restrict__ directions, int64_t n,
                     int32_t max_cells, double *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  const double origin[3] = {ox, oy, oz};
  const SkyRay ray = sky_load_ray(directions, k);
  double *o = out + k * (3 + 2 * (int64_t)max_cells);
  double pos[3], t_start, t_out;
  int32_t index[3];
  if (!sky_ray_start(g, origin, ray, pos, index, t_start, t_out)) {
    o[0] = __builtin_nan("");
    o[1] = __builtin_nan("");
    o[2] = 0.;
    return;
  }
  int steps = 0;
  while (line_image_inside(g, index)) {
    const int64_t cell =
        ((int64_t)index[0] * g.ncell[1] + index[1]) * g.ncell[2] + index[2];
    const double ds = sky_step(g, ray, pos, index);
    if (steps < max_cells) {
      o[3 + steps] = (double)cell;
      o[3 + max_cells + steps] = ds;
    }
    ++steps;
  }
  o[0] = t_start;
  o[1] = t_out;
  o[2] = (double)steps;
}

#endif
