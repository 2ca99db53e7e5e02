/*
 * line_cube_kernels.h - spectral line cubes: the emission-line images of
 * line_image_kernels.h resolved in radial velocity (include/cmi_gpu.h,
 * "spectral line cubes", has the contract). The ray geometry, the march order
 * and the cell and path-length arithmetic are the images' (ray_walk.h); what
 * is new is that a step's contribution is spread over the velocity channels
 * its Gaussian overlaps.
 *
 * Velocity axis: nchan channels of equal width over [vmin, vmax), edge
 *   e_c = vmin + c * dv,  dv = (vmax - vmin) / nchan,  c = 0 .. nchan
 * in exactly this form (no contraction: -ffp-contract=off). A cell of
 * velocity v has the radial velocity u = -((v_x n_x + v_y n_y) + v_z n_z),
 * positive for matter that recedes, and the width b = sqrt(2) sigma. The
 * fraction of its emission in channel c is
 *   f_c = 0.5 * (E((e_{c+1} - u) / b) - E((e_c - u) / b)),
 *   E(z) = 1 for z >= 6, erf(z) for -6 < z < 6, -1 otherwise.
 * "Otherwise" includes NaN, and that is how b == 0 is the step function with
 * the lower edge inclusive without a special case: (e - u) / 0 is +inf above
 * u, -inf below it and NaN (0 / 0) at e == u, which gives -1, so that a delta
 * line at u == e_c belongs to channel c. cube_E is written with ordered
 * comparisons only; the build has no fast-math flag that would let the
 * compiler assume there are no NaNs.
 *
 * Records: {k, u, s_0, b_0, .. s_{L-1}, b_{L-1}} per cell, fp64, 16 (1 + L)
 * bytes, L <= CMI_LINE_IMAGE_BATCH; k and s as in the images' records. A
 * march of line l loads the pairs {k, u} and {s_l, b_l} as two double2.
 *
 * Per step of length ds, the product in parentheses formed first, exactly as
 * the image kernel forms it:
 *   k == 0:  I_c += (s ds) f_c
 *   else:    dtau = k ds;  I_c = I_c exp(-dtau) + (s * -expm1(-dtau)) f_c
 * With one channel that covers u +- 6 b of every cell f_0 = 0.5 * (1 - -1) =
 * 1 and the cube is the image, bit for bit.
 *
 * Mapping: the images' (one lane per sample ray, 8 x 8 wave tiles, 2 x 2
 * waves per workgroup); a launch handles one block of CB consecutive
 * channels (blockIdx.y selects the line of the batch), with the CB
 * accumulators in registers, and the march is repeated per channel block. A
 * lane whose cell has all of its block's edges on one side of the clamp (z_hi
 * <= -6, or z_lo >= 6; f_c == 0 exactly for the whole block) only attenuates;
 * otherwise E is evaluated at the block's edges, each interior edge once. No
 * atomics, no LDS, no read-modify-write of memory: the same call gives the
 * same bits. DESIGN.md 4.12 has the figures.
 */
#ifndef CMI_LINE_CUBE_KERNELS_H
#define CMI_LINE_CUBE_KERNELS_H

#include "line_image_kernels.h"

/* channels per march launch */
#ifndef CMI_LINE_CUBE_CB
#define CMI_LINE_CUBE_CB 8
#endif

/* standard atomic weights of the emitting elements, per emission line; 0: the
 * entry is not a single-ion line and has no cube (HII, the Balmer jumps, the
 * averages, Hrec_s and the WFC2 filters). Host side: the record kernel gets
 * the weights of its batch by value. */
static const double cmi_emission_atomic_weight[CMI_NEMISSIONLINE] = {
    /* HAlpha, HBeta */ 1.00794, 1.00794,
    /* HII, BALMER_JUMP_LOW, BALMER_JUMP_HIGH */ 0., 0., 0.,
    /* OI_6300, OI_6364, OII_3727 */ 15.9994, 15.9994, 15.9994,
    /* OIII_5007, _4959, _4363, _52mu, _88mu */
    15.9994, 15.9994, 15.9994, 15.9994, 15.9994,
    /* NII_5755, NII_6548, NII_6584 */ 14.0067, 14.0067, 14.0067,
    /* NeIII_3869, NeIII_3968 */ 20.1797, 20.1797,
    /* SII_6725, SII_4072 */ 32.065, 32.065,
    /* SIII_9405, _6312, _19mu, _33mu */ 32.065, 32.065, 32.065, 32.065,
    /* avg_T, avg_T_count, avg_nH_nHe, avg_nH_nHe_count */ 0., 0., 0., 0.,
    /* NeII_12mu, NIII_57mu, NeIII_15mu, NII_122mu */
    20.1797, 14.0067, 20.1797, 14.0067,
    /* CII_158mu, CII_2325, CIII_1908 */ 12.0107, 12.0107, 12.0107,
    /* OII_7325, SIV_10mu, HeI_5876 */ 15.9994, 32.065, 4.002602,
    /* Hrec_s, WFC2_F439W, WFC2_F555W, WFC2_F675W */ 0., 0., 0., 0.};

/* the clamped error function of the contract; NaN gives -1 (see above). Not
 * inlined on purpose: CB + 1 inlined copies of erf's polynomials raise the
 * march kernel from 127 to 149 VGPRs at CB = 8 (181 at CB = 16), one wave per
 * SIMD less, for the price of one call per edge next to some hundred fp64
 * operations. */
__device__ __attribute__((noinline)) double cube_E(double z) {
  return (z >= 6.) ? 1. : ((z > -6.) ? erf(z) : -1.);
}

/* u of a cell: velocity is [3][ncell] on the device, or null (at rest) */
__device__ __forceinline__ double cube_radial_velocity(
    const double *__restrict__ velocity, int64_t ncell, int64_t c,
    const double n[3]) {
  if (!velocity)
    return 0.;
  return -((velocity[c] * n[0] + velocity[ncell + c] * n[1]) +
           velocity[2 * ncell + c] * n[2]);
}

/* one record from a cell's extinction coefficient, radial velocity,
 * emissivities and widths */
__device__ __forceinline__ void line_cube_store_record(double *rec, double k,
                                                       double u,
                                                       const double *j,
                                                       const double *b,
                                                       int nlines) {
  double2 *dst = reinterpret_cast<double2 *>(rec);
  dst[0] = make_double2(k, u);
  for (int l = 0; l < nlines; ++l) {
    const double q = j[l] / (4. * M_PI);
    dst[1 + l] = make_double2((k == 0.) ? q : q / k, b[l]);
  }
}

struct LineCubeRecordArgs {
  ModelDev model;
  CellsDev cells;
  int64_t ncell;
  int32_t nlines;
  int32_t lines[CMI_LINE_IMAGE_BATCH];
  double weight[CMI_LINE_IMAGE_BATCH]; /* atomic weights A of the lines */
  double dust_cross_section;           /* m^2 per hydrogen nucleus */
  double sigma_turb;                   /* m s^-1 */
  double n[3];                         /* to the observer */
  const double *velocity;              /* [3][ncell] or null */
  double *records;                     /* [ncell][2 + 2 nlines] */
};

/* records of a batch of emission lines from the cells as they are: the
 * emissivities once per cell for the whole batch; b = sqrt(2 (k_B T / (A m_u)
 * + sigma_turb^2)) */
__global__ void __launch_bounds__(CMI_BLOCK)
    line_cube_record_kernel(const LineCubeRecordArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int nd = 2 + 2 * a.nlines;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    double x[CMI_NION], values[CMI_NEMISSIONLINE];
#pragma unroll
    for (int i = 0; i < CMI_NION; ++i)
      x[i] = a.cells.x[i][c];
    const double ntot = a.cells.number_density[c];
    const double T = a.cells.temperature[c];
    cell_emissivities(a.model, ntot, T, x, values);
    double j[CMI_LINE_IMAGE_BATCH], b[CMI_LINE_IMAGE_BATCH];
    for (int l = 0; l < CMI_LINE_IMAGE_BATCH; ++l) {
      j[l] = l < a.nlines ? values[a.lines[l]] : 0.;
      b[l] = l < a.nlines
                 ? sqrt(2. * (CMI_BOLTZMANN * T /
                                  (a.weight[l] * CMI_ATOMIC_MASS_UNIT) +
                              a.sigma_turb * a.sigma_turb))
                 : 0.;
    }
    line_cube_store_record(a.records + c * nd, ntot * a.dust_cross_section,
                           cube_radial_velocity(a.velocity, a.ncell, c, a.n),
                           j, b, a.nlines);
  }
}

/* records of a batch of caller-supplied fields and widths ([nfields][ncell]
 * on the device); extinction and velocity may be null */
__global__ void __launch_bounds__(256)
    field_cube_record_kernel(const double *__restrict__ fields,
                             const double *__restrict__ widths,
                             const double *__restrict__ extinction,
                             const double *__restrict__ velocity, double n0,
                             double n1, double n2, int64_t ncell,
                             int32_t nfields, double *__restrict__ records) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell)
    return;
  double j[CMI_LINE_IMAGE_BATCH], b[CMI_LINE_IMAGE_BATCH];
  for (int l = 0; l < CMI_LINE_IMAGE_BATCH; ++l) {
    j[l] = l < nfields ? fields[(int64_t)l * ncell + c] : 0.;
    b[l] = l < nfields ? widths[(int64_t)l * ncell + c] : 0.;
  }
  const double n[3] = {n0, n1, n2};
  line_cube_store_record(records + c * (2 + 2 * nfields),
                         extinction ? extinction[c] : 0.,
                         cube_radial_velocity(velocity, ncell, c, n), j, b,
                         nfields);
}

/* the number of values that are not finite, added to *ninvalid (in the style
 * of cell_source_check_kernel: one atomic per wave that found any; the count
 * does not depend on the order) */
__global__ void __launch_bounds__(256)
    cell_velocity_check_kernel(const double *__restrict__ values, int64_t n,
                               unsigned int *ninvalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n;
       c += stride)
    bad += (fabs(values[c]) < HUGE_VAL) ? 0u : 1u;
  for (int off = 32; off > 0; off >>= 1)
    bad += __shfl_down(bad, off, 64);
  if (threadIdx.x % 64 == 0 && bad)
    atomicAdd(ninvalid, bad);
}

struct LineCubeMarchArgs {
  GridDev grid;
  LineViewDev view;
  const double *records; /* [ncell][nd] */
  int32_t nd;            /* doubles per record, 2 + 2 L */
  /* sample rows [sx0, sx1) of the sample grid, as in LineMarchArgs */
  int32_t sx0, sx1;
  /* channels [c0, c0 + nc) of nchan, nc <= CB */
  int32_t c0, nc;
  double vmin, dv;
  /* sample (sx, sy) of channel c0 + i of line l = blockIdx.y goes to
   * out[l * line_stride + i * channel_stride + (sx - sx0) * ny s + sy] */
  int64_t line_stride, channel_stride;
  double *out;
};

/* the march of one line and one block of CB channels: one lane per sample
 * ray, far side to near side */
template <int CB>
__global__ void __launch_bounds__(256)
    line_cube_march_kernel(const LineCubeMarchArgs a) {
  int32_t sx, sy;
  double x, y;
  if (!tile_sample(a.view, a.sx0, a.sx1, sx, sy, x, y))
    return;
  const int32_t line = blockIdx.y;

  double edge[CB + 1];
  channel_block_edges<CB>(a.vmin, a.dv, a.c0, a.nc, edge);

  double I[CB];
#pragma unroll
  for (int i = 0; i < CB; ++i)
    I[i] = 0.;
  GridRay ray;
  if (ray.start(a.grid, a.view, x, y)) {
    while (ray.inside(a.grid)) {
      const double2 *rec = reinterpret_cast<const double2 *>(
          a.records + ray.cell(a.grid) * a.nd);
      const double2 ku = rec[0];
      const double2 sb = rec[1 + line];
      const double ds = ray.step(a.grid);
      const double k = ku.x, u = ku.y, s = sb.x, b = sb.y;
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
      if (dark) {
        if (k != 0.) {
#pragma unroll
          for (int i = 0; i < CB; ++i)
            I[i] = I[i] * att;
        }
      } else {
        double E_lo = cube_E(z_lo);
#pragma unroll
        for (int i = 0; i < CB; ++i) {
          const double E_hi = cube_E((edge[i + 1] - u) / b);
          const double f = 0.5 * (E_hi - E_lo);
          if (k == 0.)
            I[i] += w * f;
          else
            I[i] = I[i] * att + w * f;
          E_lo = E_hi;
        }
      }
    }
  }
  const int64_t at = tile_sample_at(a.view, a.sx0, sx, sy);
  double *out = a.out + line * a.line_stride + at;
#pragma unroll
  for (int i = 0; i < CB; ++i)
    if (i < a.nc)
      out[i * a.channel_stride] = I[i];
}

#endif
