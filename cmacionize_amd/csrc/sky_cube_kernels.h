/*
 * sky_cube_kernels.h - sky cubes: the sky maps of sky_image_kernels.h
 * resolved in radial velocity (include/cmi_gpu.h, "sky cubes", has the
 * contract). The rays, the slab test, the start cell and the step are the sky
 * maps' (ray_walk.h); the velocity axis, E and f_c are the spectral line
 * cubes' (channel_block_edges, cube_E). What is
 * new is the radial velocity: every ray has a direction of its own, so a
 * cell's u is not a property of the cell. The records carry the cell's
 * velocity relative to the observer, w = v - v_obs, and a lane forms
 *   u = (w_x d_x + w_y d_y) + w_z d_z
 * with its own d (no contraction), positive for matter that recedes: d points
 * away from the observer.
 *
 * Records: {k, w_x, w_y, w_z, s_0, b_0, .. s_{L-1}, b_{L-1}} per cell, fp64,
 * 32 + 16 L bytes, L <= CMI_SKY_CUBE_BATCH = 6 (one 128-B line); k and s as
 * in the images' records, b as in the cubes'. A march of line l loads
 * {k, w_x}, {w_y, w_z} and {s_l, b_l} as three double2.
 *
 * Per step of length ds, observer outwards, T = 1 and I_c = 0 at the start:
 *   k == 0:  I_c += T * ((s * ds) * f_c)
 *   else:    dtau = k * ds;  I_c += T * ((s * -expm1(-dtau)) * f_c);
 *            T = T * exp(-dtau)
 * in this order of multiplications: with f_c == 1 these are the bits of
 * sky_march_kernel.
 *
 * Mapping: one lane per ray in the caller's order (the sky maps'), blockIdx.y
 * the line of the batch; a launch handles one block of CB consecutive
 * channels with the CB accumulators in registers, and the march is repeated
 * per channel block. A lane whose cell is dark for the whole block (!(z_hi >
 * -6) || z_lo >= 6; f_c == 0 exactly) updates T only: observer outwards
 * there is nothing to attenuate, and I_c + T * (w * 0) is I_c, so the
 * shortcut gives the bits of the full update. No atomics, no LDS, no
 * read-modify-write of memory: the same call gives the same bits. DESIGN.md
 * 4.13 has the figures.
 */
#ifndef CMI_SKY_CUBE_KERNELS_H
#define CMI_SKY_CUBE_KERNELS_H

#include "line_cube_kernels.h"
#include "sky_image_kernels.h"

/* lines per record: 32 + 16 L <= 128 B */
#define CMI_SKY_CUBE_BATCH 6

/* channels per march launch */
#ifndef CMI_SKY_CUBE_CB
#define CMI_SKY_CUBE_CB 8
#endif

/* one record from a cell's extinction coefficient, velocity relative to the
 * observer, emissivities and widths */
__device__ __forceinline__ void sky_cube_store_record(double *rec, double k,
                                                      const double w[3],
                                                      const double *j,
                                                      const double *b,
                                                      int nlines) {
  double2 *dst = reinterpret_cast<double2 *>(rec);
  dst[0] = make_double2(k, w[0]);
  dst[1] = make_double2(w[1], w[2]);
  for (int l = 0; l < nlines; ++l) {
    const double q = j[l] / (4. * M_PI);
    dst[2 + l] = make_double2((k == 0.) ? q : q / k, b[l]);
  }
}

/* w of a cell: velocity is [3][ncell] on the device, or null (at rest) */
__device__ __forceinline__ void sky_cube_relative_velocity(
    const double *__restrict__ velocity, int64_t ncell, int64_t c,
    const double v_obs[3], double w[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    w[a] = (velocity ? velocity[a * ncell + c] : 0.) - v_obs[a];
}

struct SkyCubeRecordArgs {
  ModelDev model;
  CellsDev cells;
  int64_t ncell;
  int32_t nlines;
  int32_t lines[CMI_SKY_CUBE_BATCH];
  double weight[CMI_SKY_CUBE_BATCH]; /* atomic weights A of the lines */
  double dust_cross_section;         /* m^2 per hydrogen nucleus */
  double sigma_turb;                 /* m s^-1 */
  double v_obs[3];                   /* m s^-1 */
  const double *velocity;            /* [3][ncell] or null */
  double *records;                   /* [ncell][4 + 2 nlines] */
};

/* records of a batch of emission lines from the cells as they are: the
 * emissivities once per cell for the whole batch; b as in
 * line_cube_record_kernel */
__global__ void __launch_bounds__(CMI_BLOCK)
    sky_cube_record_kernel(const SkyCubeRecordArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int nd = 4 + 2 * a.nlines;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    double x[CMI_NION], values[CMI_NEMISSIONLINE];
#pragma unroll
    for (int i = 0; i < CMI_NION; ++i)
      x[i] = a.cells.x[i][c];
    const double ntot = a.cells.number_density[c];
    const double T = a.cells.temperature[c];
    cell_emissivities(a.model, ntot, T, x, values);
    double j[CMI_SKY_CUBE_BATCH], b[CMI_SKY_CUBE_BATCH];
    for (int l = 0; l < CMI_SKY_CUBE_BATCH; ++l) {
      j[l] = l < a.nlines ? values[a.lines[l]] : 0.;
      b[l] = l < a.nlines
                 ? sqrt(2. * (CMI_BOLTZMANN * T /
                                  (a.weight[l] * CMI_ATOMIC_MASS_UNIT) +
                              a.sigma_turb * a.sigma_turb))
                 : 0.;
    }
    double w[3];
    sky_cube_relative_velocity(a.velocity, a.ncell, c, a.v_obs, w);
    sky_cube_store_record(a.records + c * nd, ntot * a.dust_cross_section, w,
                          j, b, a.nlines);
  }
}

/* records of a batch of caller-supplied fields and widths ([nfields][ncell]
 * on the device); extinction and velocity may be null */
__global__ void __launch_bounds__(256)
    field_sky_cube_record_kernel(const double *__restrict__ fields,
                                 const double *__restrict__ widths,
                                 const double *__restrict__ extinction,
                                 const double *__restrict__ velocity,
                                 double vo0, double vo1, double vo2,
                                 int64_t ncell, int32_t nfields,
                                 double *__restrict__ records) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell)
    return;
  double j[CMI_SKY_CUBE_BATCH], b[CMI_SKY_CUBE_BATCH];
  for (int l = 0; l < CMI_SKY_CUBE_BATCH; ++l) {
    j[l] = l < nfields ? fields[(int64_t)l * ncell + c] : 0.;
    b[l] = l < nfields ? widths[(int64_t)l * ncell + c] : 0.;
  }
  const double v_obs[3] = {vo0, vo1, vo2};
  double w[3];
  sky_cube_relative_velocity(velocity, ncell, c, v_obs, w);
  sky_cube_store_record(records + c * (4 + 2 * nfields),
                        extinction ? extinction[c] : 0., w, j, b, nfields);
}

struct SkyCubeMarchArgs {
  GridDev grid;
  double origin[3];
  const double *directions; /* [nrays][3] */
  const double *records;    /* [ncell][nd] */
  int64_t nrays;
  int32_t nd; /* doubles per record, 4 + 2 L */
  /* channels [c0, c0 + nc) of nchan, nc <= CB */
  int32_t c0, nc;
  int32_t pad;
  double vmin, dv;
  /* ray r of channel c0 + i of line l = blockIdx.y goes to
   * out[l * line_stride + (c0 + i) * channel_stride + r] */
  int64_t line_stride, channel_stride;
  double *out;
};

/* the march of one line and one block of CB channels: one lane per ray,
 * observer outwards */
template <int CB>
__global__ void __launch_bounds__(256)
    sky_cube_march_kernel(const SkyCubeMarchArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrays)
    return;
  const int32_t line = blockIdx.y;
  double edge[CB + 1];
  channel_block_edges<CB>(a.vmin, a.dv, a.c0, a.nc, edge);

  double I[CB];
#pragma unroll
  for (int i = 0; i < CB; ++i)
    I[i] = 0.;
  double T = 1.;
  GridRay ray;
  if (ray.start(a.grid, a.origin, a.directions, r)) {
    while (ray.inside(a.grid)) {
      const double2 *rec = reinterpret_cast<const double2 *>(
          a.records + ray.cell(a.grid) * a.nd);
      const double2 kw = rec[0];
      const double2 ww = rec[1];
      const double2 sb = rec[2 + line];
      const double ds = ray.step(a.grid);
      const double k = kw.x, s = sb.x, b = sb.y;
      const double u = (kw.y * ray.d[0] + ww.x * ray.d[1]) + ww.y * ray.d[2];
      double att = 1., w;
      if (k == 0.) {
        w = s * ds;
      } else {
        const double dtau = k * ds;
        att = exp(-dtau);
        w = s * -expm1(-dtau);
      }
      const double z_lo = (edge[0] - u) / b;
      const double z_hi = (edge[CB] - u) / b;
      const bool dark = channel_block_dark(z_lo, z_hi);
      if (!dark) {
        double E_lo = cube_E(z_lo);
#pragma unroll
        for (int i = 0; i < CB; ++i) {
          const double E_hi = cube_E((edge[i + 1] - u) / b);
          const double f = 0.5 * (E_hi - E_lo);
          I[i] += T * (w * f);
          E_lo = E_hi;
        }
      }
      if (k != 0.)
        T = T * att;
    }
  }
  double *out = a.out + line * a.line_stride + a.c0 * a.channel_stride + r;
#pragma unroll
  for (int i = 0; i < CB; ++i)
    if (i < a.nc)
      out[i * a.channel_stride] = I[i];
}

#endif
