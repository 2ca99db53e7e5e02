/*
 * sky_image_kernels.h - sky maps: line images for an observer inside or near
 * the grid. line_image_kernels.h sees the box from infinitely far away, one
 * direction for all rays; here every ray leaves one point, the origin o, in
 * a direction of its own, and the integration runs from the observer
 * outwards, carrying the transmission. The records, the units and the
 * discipline of a CPU restatement (tests/support/sky_image_reference.c) are
 * those of line_image_kernels.h.
 *
 * The rays, their cells and the path lengths are ray_walk.h's (GridRay with
 * the point camera's start).
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
  double I[ND - 1];
#pragma unroll
  for (int l = 0; l < ND - 1; ++l)
    I[l] = 0.;
  double T = 1.;
  GridRay ray;
  if (ray.start(a.grid, a.origin, a.directions, r)) {
    while (ray.inside(a.grid)) {
      const double2 *rec = reinterpret_cast<const double2 *>(
          a.records + ray.cell(a.grid) * ND);
      double rc[ND];
#pragma unroll
      for (int h = 0; h < ND / 2; ++h) {
        const double2 w = rec[h];
        rc[2 * h] = w.x;
        rc[2 * h + 1] = w.y;
      }
      const double ds = ray.step(a.grid);
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
  double *o = out + k * (3 + 2 * (int64_t)max_cells);
  GridRay ray;
  const bool hit = ray.start(g, origin, directions, k);
  probe_row(g, ray, hit, max_cells, o, [](int64_t, double, int) {});
}

#endif
