/*
 * continuum_kernels.h - continuum images: the formal solution of the transfer
 * equation with an absorption coefficient and a source function of their own
 * in every channel (include/cmi_gpu.h, "continuum images", has the contract;
 * DESIGN.md 4.15 the reasoning). The line products share one grey exp(-k ds)
 * among their channels and emit what the cell does not absorb itself; here a
 * channel f has kappa_f (m^-1) and S_f (W m^-2 Hz^-1 sr^-1) per cell and the
 * cell absorbs its own emission. The rays, the cells and the path lengths are
 * the images' and the sky maps' (ray_walk.h).
 *
 * Records: FB pairs {kappa_f, S_f} per cell as double2, 16 FB bytes, for one
 * block of FB consecutive channels; the slots past the last channel of a
 * partial block hold {0, 0}.
 *
 * Parallel camera, far side to near side, I_f = bg_f at the start (and for a
 * ray that misses the box); per cell with path ds
 *   em = expm1(-(kappa_f * ds));  I_f = I_f + em * (I_f - S_f)
 * kappa == 0 gives em == 0 and leaves I_f as it is; I_f == S_f gives a
 * difference of exactly 0 and leaves it too.
 *
 * Rays from a point, observer outwards, T_f = 1 and I_f = 0 at the start; per
 * cell
 *   em = expm1(-(kappa_f * ds));  I_f = I_f + T_f * (S_f * -em);
 *   T_f = T_f + T_f * em
 * and after the last cell, or for a ray that misses, I_f = I_f + T_f * bg_f.
 *
 * One expm1 per cell and channel and no exp: 1 - e^-tau and e^-tau - 1 are the
 * same number, so that the attenuation and the emission cannot disagree, and
 * expm1 keeps the thin limit (tau = 1e-12) to the last bit where 1 - exp
 * would cancel.
 *
 * Mapping: the line cubes' (one lane per sample ray, 8 x 8 wave tiles, 2 x 2
 * waves per workgroup) and the sky cubes' (one lane per ray in the caller's
 * order); a launch marches one block of FB channels with its accumulators in
 * registers (FB for the parallel camera, 2 FB for the rays from a point). No
 * atomics, no LDS, no read-modify-write of memory: the same call gives the
 * same bits, and a channel's bits do not depend on the block it is in.
 *
 * Free-free coefficients of the cells as they are (free_free_pair): Draine
 * (2011) eq. 10.1 and 10.9 for the emissivity, B_nu(T) for the source
 * function and Kirchhoff's law kappa = j / S for the opacity.
 */
#ifndef CMI_CONTINUUM_KERNELS_H
#define CMI_CONTINUUM_KERNELS_H

#include "line_cube_kernels.h"
#include "sky_image_kernels.h"

/* the widest channel block that is built (FB is 4, 8 or 16) */
#define CMI_CONTINUUM_MAX_FB 16
/* channels per march launch unless the tuning key continuum_channel_block
 * says otherwise (DESIGN.md 4.15 has the measurement) */
#ifndef CMI_CONTINUUM_FB
#define CMI_CONTINUUM_FB 8
#endif

/* 5.444364709e-39 erg cm^3 s^-1 Hz^-1 sr^-1 K^1/2, the Gaussian (2^5 pi e^6 /
 * (3 m_e c^3)) sqrt(2 pi / (3 k m_e)) / (4 pi), times 1e-13 for W and m^-3 */
#define CMI_FREE_FREE_EMISSIVITY 5.444364709e-52

/* {kappa, S} of thermal free-free emission at the frequency nu (Hz) of a cell
 * of n nuclei of hydrogen per m^3 at T (K) with the neutral fractions x_H0
 * and x_He0 and the helium abundance A_He; ions of charge 1 only. A cell
 * without electrons, without a temperature or whose B_nu underflows has
 * {0, 0} exactly. */
__device__ __forceinline__ double2 free_free_pair(double n, double T,
                                                  double x_H0, double x_He0,
                                                  double A_He, double nu) {
  const double n_e = n * ((1. - x_H0) + A_He * (1. - x_He0));
  if (n_e == 0. || !(T > 0.))
    return make_double2(0., 0.);
  const double x = (CMI_PLANCK * nu) / (CMI_BOLTZMANN * T);
  const double S = (2. * CMI_PLANCK * nu * nu * nu /
                    (CMI_LIGHTSPEED * CMI_LIGHTSPEED)) /
                   expm1(x);
  if (S == 0.)
    return make_double2(0., 0.);
  const double g =
      log(exp(5.960 - (sqrt(3.) / M_PI) *
                          log((nu / 1.e9) * pow(T / 1.e4, -1.5))) +
          M_E);
  const double n_i = n_e;
  const double j =
      CMI_FREE_FREE_EMISSIVITY * g * n_e * n_i / sqrt(T) * exp(-x);
  return make_double2(j / S, S);
}

struct FreeFreeRecordArgs {
  CellsDev cells;
  int64_t ncell;
  double helium_abundance;
  int32_t fb;    /* pairs per record */
  int32_t nfreq; /* frequencies of this block, <= fb */
  double freq[CMI_CONTINUUM_MAX_FB];
  double *records; /* [ncell][fb] pairs */
};

/* records of a block of frequencies from the cells as they are */
__global__ void __launch_bounds__(256)
    free_free_record_kernel(const FreeFreeRecordArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    const double n = a.cells.number_density[c];
    const double T = a.cells.temperature[c];
    const double x_H0 = a.cells.x[0][c], x_He0 = a.cells.x[1][c];
    double2 *dst = reinterpret_cast<double2 *>(a.records) + c * a.fb;
    /* (unrolled over the widest block: a.freq is indexed at compile time) */
#pragma unroll
    for (int f = 0; f < CMI_CONTINUUM_MAX_FB; ++f)
      if (f < a.fb)
        dst[f] = (f < a.nfreq) ? free_free_pair(n, T, x_H0, x_He0,
                                                a.helium_abundance, a.freq[f])
                               : make_double2(0., 0.);
  }
}

/* records of a block of nf <= fb caller-supplied channels: kappa[nf][ncell],
 * source[nf][ncell] on the device */
__global__ void __launch_bounds__(256)
    field_continuum_record_kernel(const double *__restrict__ kappa,
                                  const double *__restrict__ source,
                                  int64_t ncell, int32_t nf, int32_t fb,
                                  double *__restrict__ records) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell)
    return;
  double2 *dst = reinterpret_cast<double2 *>(records) + c * fb;
  for (int f = 0; f < fb; ++f)
    dst[f] = (f < nf) ? make_double2(kappa[(int64_t)f * ncell + c],
                                     source[(int64_t)f * ncell + c])
                      : make_double2(0., 0.);
}

/* the number of absorption coefficients that are negative or not finite,
 * added to ninvalid[0], and of source functions that are not finite, added to
 * ninvalid[1] (in the style of cell_velocity_check_kernel: one atomic per
 * wave that found any; the counts do not depend on the order) */
__global__ void __launch_bounds__(256)
    continuum_field_check_kernel(const double *__restrict__ kappa,
                                 const double *__restrict__ source, int64_t n,
                                 unsigned int *ninvalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad_k = 0, bad_s = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n;
       c += stride) {
    const double k = kappa[c];
    bad_k += (k >= 0. && k < HUGE_VAL) ? 0u : 1u;
    bad_s += (fabs(source[c]) < HUGE_VAL) ? 0u : 1u;
  }
  for (int off = 32; off > 0; off >>= 1) {
    bad_k += __shfl_down(bad_k, off, 64);
    bad_s += __shfl_down(bad_s, off, 64);
  }
  if (threadIdx.x % 64 == 0) {
    if (bad_k)
      atomicAdd(ninvalid, bad_k);
    if (bad_s)
      atomicAdd(ninvalid + 1, bad_s);
  }
}

struct ContinuumMarchArgs {
  GridDev grid;
  LineViewDev view;
  const double *records; /* [ncell][FB] pairs */
  /* sample rows [sx0, sx1) of the sample grid, as in LineMarchArgs */
  int32_t sx0, sx1;
  int32_t nc; /* channels of this block, <= FB */
  int32_t pad;
  /* sample (sx, sy) of the block's channel i goes to
   * out[i * channel_stride + (sx - sx0) * ny s + sy] */
  int64_t channel_stride;
  double *out;
  double background[CMI_CONTINUUM_MAX_FB]; /* of the block's channels */
};

/* the march of one block of FB channels: one lane per sample ray, far side to
 * near side */
template <int FB>
__global__ void __launch_bounds__(256)
    continuum_march_kernel(const ContinuumMarchArgs a) {
  int32_t sx, sy;
  double x, y;
  if (!tile_sample(a.view, a.sx0, a.sx1, sx, sy, x, y))
    return;

  double I[FB];
#pragma unroll
  for (int i = 0; i < FB; ++i)
    I[i] = a.background[i];
  GridRay ray;
  if (ray.start(a.grid, a.view, x, y)) {
    while (ray.inside(a.grid)) {
      const double2 *rec =
          reinterpret_cast<const double2 *>(a.records) + ray.cell(a.grid) * FB;
      double2 ks[FB];
#pragma unroll
      for (int i = 0; i < FB; ++i)
        ks[i] = rec[i];
      const double ds = ray.step(a.grid);
#pragma unroll
      for (int i = 0; i < FB; ++i) {
        /* (the slots past a partial block hold {0, 0}: em == 0) */
        const double em = expm1(-(ks[i].x * ds));
        I[i] = I[i] + em * (I[i] - ks[i].y);
      }
    }
  }
  const int64_t at = tile_sample_at(a.view, a.sx0, sx, sy);
#pragma unroll
  for (int i = 0; i < FB; ++i)
    if (i < a.nc)
      a.out[i * a.channel_stride + at] = I[i];
}

struct ContinuumSkyMarchArgs {
  GridDev grid;
  double origin[3];
  const double *directions; /* [nrays][3] */
  const double *records;    /* [ncell][FB] pairs */
  int64_t nrays;
  int32_t nc; /* channels of this block, <= FB */
  int32_t pad;
  /* ray r of the block's channel i goes to out[i * channel_stride + r] */
  int64_t channel_stride;
  double *out;
  double background[CMI_CONTINUUM_MAX_FB]; /* of the block's channels */
};

/* the march of one block of FB channels: one lane per ray, observer
 * outwards */
template <int FB>
__global__ void __launch_bounds__(256)
    continuum_sky_march_kernel(const ContinuumSkyMarchArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrays)
    return;
  double I[FB], T[FB];
#pragma unroll
  for (int i = 0; i < FB; ++i) {
    I[i] = 0.;
    T[i] = 1.;
  }
  GridRay ray;
  if (ray.start(a.grid, a.origin, a.directions, r)) {
    while (ray.inside(a.grid)) {
      const double2 *rec =
          reinterpret_cast<const double2 *>(a.records) + ray.cell(a.grid) * FB;
      double2 ks[FB];
#pragma unroll
      for (int i = 0; i < FB; ++i)
        ks[i] = rec[i];
      const double ds = ray.step(a.grid);
#pragma unroll
      for (int i = 0; i < FB; ++i) {
        const double em = expm1(-(ks[i].x * ds));
        I[i] = I[i] + T[i] * (ks[i].y * -em);
        T[i] = T[i] + T[i] * em;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < FB; ++i)
    if (i < a.nc)
      a.out[i * a.channel_stride + r] = I[i] + T[i] * a.background[i];
}

/* row k of continuum_probe_kernel with the camera chosen */
template <bool POINT>
__device__ __forceinline__ void continuum_probe_row(
    const GridDev &g, const LineViewDev &v, const double origin[3],
    const double *__restrict__ rays, int64_t k,
    const double *__restrict__ kappa, const double *__restrict__ source,
    const double *__restrict__ background, int32_t nf, int64_t ncell,
    int32_t max_cells, double *o) {
  double *I_steps = o + 3 + 2 * (int64_t)max_cells;
  double *I_end = I_steps + (int64_t)nf * max_cells;
  for (int32_t f = 0; f < nf; ++f) {
    const double bg = background[f];
    GridRay ray;
    const bool hit = POINT ? ray.start(g, origin, rays, k)
                           : ray.start(g, v, rays[2 * k], rays[2 * k + 1]);
    double I = POINT ? 0. : bg, T = 1.;
    /* (the geometry is every channel's: each writes the same prefix) */
    probe_row(g, ray, hit, max_cells, o, [&](int64_t cell, double ds, int i) {
      const double kf = kappa[(int64_t)f * ncell + cell];
      const double sf = source[(int64_t)f * ncell + cell];
      const double em = expm1(-(kf * ds));
      if (POINT) {
        I = I + T * (sf * -em);
        T = T + T * em;
      } else {
        I = I + em * (I - sf);
      }
      if (i < max_cells)
        I_steps[(int64_t)f * max_cells + i] = I;
    });
    I_end[f] = POINT ? I + T * bg : I;
  }
}

/* cmi_gpu_continuum_probe: row k = {t0, t1, steps, cells[max_cells],
 * ds[max_cells], I[nf][max_cells], I_end[nf]} of ray k; I[f][i] is I_f after
 * step i (before the background is added, for the rays from a point) and
 * I_end what the march kernels store. kappa and source are [nf][ncell] on the
 * device, background [nf]. One channel at a time: the probe is not a hot
 * path, and a channel's arithmetic is the march kernels' operation for
 * operation. point == 0: the parallel camera, rays[k] = {x, y}; otherwise
 * rays from o, rays[k] = the direction. */
__global__ void __launch_bounds__(64)
    continuum_probe_kernel(GridDev g, LineViewDev v, int32_t point, double ox,
                           double oy, double oz,
                           const double *__restrict__ rays, int64_t n,
                           const double *__restrict__ kappa,
                           const double *__restrict__ source,
                           const double *__restrict__ background, int32_t nf,
                           int64_t ncell, int32_t max_cells,
                           double *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  double *o = out + k * (3 + (2 + (int64_t)nf) * max_cells + nf);
  const double origin[3] = {ox, oy, oz};
  if (point)
    continuum_probe_row<true>(g, v, origin, rays, k, kappa, source, background,
                              nf, ncell, max_cells, o);
  else
    continuum_probe_row<false>(g, v, origin, rays, k, kappa, source,
                               background, nf, ncell, max_cells, o);
}

#endif
