/*
 * absorbing_cube_kernels.h - absorbing line cubes: a spectral line whose
 * opacity has the line profile, in front of, behind and inside a continuum
 * (include/cmi_gpu.h, "absorbing line cubes", has the contract; DESIGN.md
 * 4.16 the reasoning), and the 21-cm line of neutral hydrogen as its first
 * client. The line cubes (line_cube_kernels.h, sky_cube_kernels.h) resolve
 * emission in velocity but share one grey exp(-k ds) among their channels; the
 * continuum images (continuum_kernels.h) have an opacity and a source function
 * per channel but no profile. Here a cell has
 *   a   the line opacity integrated over velocity, m^-1 m s^-1,
 *   sl  the line source function,
 *   b   the Gaussian width sqrt(2) sigma, u its radial velocity,
 *   kc, sc  a continuum opacity and source function, constant over the band,
 * and channel c of width dv, which holds the fraction f_c of the profile
 * (cube_E, unchanged), has per step of length ds
 *   al = (a / dv) * f_c;  kappa = al + kc
 *   kappa == 0: nothing
 *   w = al / kappa;  S = sc + w * (sl - sc);  em = expm1(-(kappa * ds))
 *   parallel camera, far to near:   I = I + em * (I - S)
 *   rays from a point, outwards:    I = I + T * (S * -em);  T = T + T * em
 * the continuum images' two updates. a == 0 gives kappa == kc and S == sc, the
 * bits of continuum_march_kernel; sl == sc == I stays I.
 *
 * Records: one per cell and call (nothing in them depends on the channel),
 * fp64 pairs loaded as double2:
 *   parallel camera, 48 B:      {a / dv, u}, {b, sl}, {kc, sc}
 *   rays from a point, 64 B:    {a / dv, w_x}, {w_y, w_z}, {b, sl}, {kc, sc}
 * with w = v - v_obs as in the sky cubes; a lane forms u with its own d.
 *
 * Mapping: the line cubes' and the sky cubes' (one lane per sample ray, 8 x 8
 * wave tiles, 2 x 2 waves per workgroup; one lane per ray in the caller's
 * order); a launch marches one block of CB consecutive channels with its CB
 * (2 CB from a point) accumulators in registers and evaluates E at the CB + 1
 * edges, each once. Window skip: a lane whose cell is dark for the whole block
 * (!(z_hi > -6) || z_lo >= 6: every f_c == 0 exactly) has al == 0, kappa ==
 * kc and S == sc + 0 * (sl - sc) in every channel, so that one expm1 serves
 * them all, and nothing at all is done when kc == 0 as well: the bits of the
 * full update (a.full != 0 runs the full update everywhere; the tests compare
 * the two). No atomics, no LDS, no read-modify-write of memory: the same call
 * gives the same bits, and a channel's bits depend on (vmin, dv, c) and the
 * cells only.
 */
#ifndef CMI_ABSORBING_CUBE_KERNELS_H
#define CMI_ABSORBING_CUBE_KERNELS_H

#include "continuum_kernels.h"
#include "sky_cube_kernels.h"

/* the widest channel block that is built (CB is 4 or 8) */
#define CMI_ABSORBING_MAX_CB 8
/* channels per march launch unless the tuning key
 * absorbing_cube_channel_block says otherwise (DESIGN.md 4.16 has the
 * measurement) */
#ifndef CMI_ABSORBING_CB
#define CMI_ABSORBING_CB 4
#endif
/* 1: the march kernels call expm1 as a function (one copy per kernel), 0:
 * they inline it per channel; the tuning key absorbing_cube_expm1_call */
#ifndef CMI_ABSORBING_EXPM1_CALL
#define CMI_ABSORBING_EXPM1_CALL 1
#endif

/* the 21-cm line: the hyperfine frequency (Hz) and its Einstein A (s^-1) */
#define CMI_HI_FREQUENCY 1420405751.768
#define CMI_HI_EINSTEIN_A 2.8843e-15

__device__ __attribute__((noinline)) double absorbing_expm1_call(double x) {
  return expm1(x);
}

template <bool CALL> __device__ __forceinline__ double absorbing_expm1(double x) {
  return CALL ? absorbing_expm1_call(x) : expm1(x);
}

/* the continuum images' update of one channel with kappa != 0 */
template <bool POINT>
__device__ __forceinline__ void absorbing_apply(double em, double S, double &I,
                                                double &T) {
  if (POINT) {
    I = I + T * (S * -em);
    T = T + T * em;
  } else {
    I = I + em * (I - S);
  }
}

/* the contract's step of one channel that holds the fraction f of the
 * profile; adv = a / dv */
template <bool POINT, bool CALL>
__device__ __forceinline__ void absorbing_channel(double adv, double f,
                                                  double sl, double kc,
                                                  double sc, double ds,
                                                  double &I, double &T) {
  const double al = adv * f;
  const double kappa = al + kc;
  if (kappa == 0.)
    return;
  const double w = al / kappa;
  const double S = sc + w * (sl - sc);
  absorbing_apply<POINT>(absorbing_expm1<CALL>(-(kappa * ds)), S, I, T);
}

/* B_nu(T) in the form of free_free_pair; 0 without a positive temperature */
__device__ __forceinline__ double absorbing_planck(double nu, double T) {
  if (!(T > 0.))
    return 0.;
  const double x = (CMI_PLANCK * nu) / (CMI_BOLTZMANN * T);
  return (2. * CMI_PLANCK * nu * nu * nu /
          (CMI_LIGHTSPEED * CMI_LIGHTSPEED)) /
         expm1(x);
}

/* one record; frame is the direction to the observer (parallel camera) or
 * the observer's velocity (rays from a point) */
template <bool POINT>
__device__ __forceinline__ void absorbing_store_record(
    double *records, int64_t c, double adv, double b, double sl, double kc,
    double sc, const double *__restrict__ velocity, int64_t ncell,
    const double frame[3]) {
  if (POINT) {
    double2 *dst = reinterpret_cast<double2 *>(records) + c * 4;
    double w[3];
    sky_cube_relative_velocity(velocity, ncell, c, frame, w);
    dst[0] = make_double2(adv, w[0]);
    dst[1] = make_double2(w[1], w[2]);
    dst[2] = make_double2(b, sl);
    dst[3] = make_double2(kc, sc);
  } else {
    double2 *dst = reinterpret_cast<double2 *>(records) + c * 3;
    dst[0] = make_double2(adv, cube_radial_velocity(velocity, ncell, c, frame));
    dst[1] = make_double2(b, sl);
    dst[2] = make_double2(kc, sc);
  }
}

/* how the spin temperature of the H I client is given */
enum { CMI_HI_SPIN_KINETIC = 0, CMI_HI_SPIN_FIXED = 1, CMI_HI_SPIN_CELLS = 2 };

struct HiRecordArgs {
  CellsDev cells;
  int64_t ncell;
  double helium_abundance;
  double weight;     /* the atomic weight of hydrogen */
  double sigma_turb; /* m s^-1 */
  double dv;         /* the channel width, m s^-1 */
  double spin_fixed; /* K, CMI_HI_SPIN_FIXED */
  const double *spin_cells; /* [ncell] K, CMI_HI_SPIN_CELLS */
  int32_t spin_mode;
  int32_t free_free;
  double frame[3];
  const double *velocity; /* [3][ncell] or null */
  double *records;
};

/* records of the 21-cm line from the cells as they are */
template <bool POINT>
__global__ void __launch_bounds__(256) hi_record_kernel(const HiRecordArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    const double n = a.cells.number_density[c];
    const double T = a.cells.temperature[c];
    const double x_H0 = a.cells.x[0][c];
    const double Ts = a.spin_mode == CMI_HI_SPIN_KINETIC ? T
                      : a.spin_mode == CMI_HI_SPIN_FIXED ? a.spin_fixed
                                                         : a.spin_cells[c];
    const double n_HI = n * x_H0;
    double al = 0.;
    if (n_HI > 0. && T > 0. && Ts > 0.)
      al = CMI_HI_COLUMN_CONSTANT * n_HI / Ts;
    const double thermal =
        (T > 0.) ? CMI_BOLTZMANN * T / (a.weight * CMI_ATOMIC_MASS_UNIT) : 0.;
    const double b = sqrt(2. * (thermal + a.sigma_turb * a.sigma_turb));
    double2 ks = make_double2(0., 0.);
    if (a.free_free)
      ks = free_free_pair(n, T, x_H0, a.cells.x[1][c], a.helium_abundance,
                          CMI_HI_FREQUENCY);
    absorbing_store_record<POINT>(a.records, c, al / a.dv, b,
                                  absorbing_planck(CMI_HI_FREQUENCY, Ts), ks.x,
                                  ks.y, a.velocity, a.ncell, a.frame);
  }
}

/* the number of records of hi_record_kernel in which a / dv, b, sl, kc, sc or
 * sl - sc is not finite, added to *ninvalid: what the caller's fields are
 * refused for (absorbing_field_check_kernel), here from cells whose numbers
 * overflow, such as a spin temperature of 1e-322 K (one atomic per wave that
 * found any) */
template <bool POINT>
__global__ void __launch_bounds__(256)
    hi_record_check_kernel(const double *__restrict__ records, int64_t ncell,
                           unsigned int *ninvalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell;
       c += stride) {
    const double2 *rec =
        reinterpret_cast<const double2 *>(records) + c * (POINT ? 4 : 3);
    const double adv = rec[0].x;
    const double2 bs = rec[POINT ? 2 : 1];
    const double2 ks = rec[POINT ? 3 : 2];
    const bool ok = fabs(adv) < HUGE_VAL && fabs(bs.x) < HUGE_VAL &&
                    fabs(bs.y) < HUGE_VAL && fabs(ks.x) < HUGE_VAL &&
                    fabs(ks.y) < HUGE_VAL && fabs(bs.y - ks.y) < HUGE_VAL;
    bad += ok ? 0u : 1u;
  }
  for (int off = 32; off > 0; off >>= 1)
    bad += __shfl_down(bad, off, 64);
  if (threadIdx.x % 64 == 0 && bad)
    atomicAdd(ninvalid, bad);
}

struct FieldAbsorbingRecordArgs {
  const double *a, *sl, *b; /* [ncell] on the device */
  const double *kc, *sc;    /* [ncell] or both null */
  const double *velocity;   /* [3][ncell] or null */
  int64_t ncell;
  double dv;
  double frame[3];
  double *records;
};

/* records of the caller's fields */
template <bool POINT>
__global__ void __launch_bounds__(256)
    field_absorbing_record_kernel(const FieldAbsorbingRecordArgs a) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.ncell)
    return;
  absorbing_store_record<POINT>(a.records, c, a.a[c] / a.dv, a.b[c], a.sl[c],
                                a.kc ? a.kc[c] : 0., a.sc ? a.sc[c] : 0.,
                                a.velocity, a.ncell, a.frame);
}

/* counts of the caller's fields that the contract refuses, added to
 * ninvalid[0 .. 4]: a negative, not finite or with a / dv not finite; b
 * negative or not finite; kc negative or not finite; sl not finite; sc not
 * finite or sl - sc not finite (in the style of continuum_field_check_kernel:
 * one atomic per wave and count that found any) */
__global__ void __launch_bounds__(256)
    absorbing_field_check_kernel(const FieldAbsorbingRecordArgs a,
                                 unsigned int *ninvalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad[5] = {0, 0, 0, 0, 0};
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    const double av = a.a[c], bv = a.b[c], sl = a.sl[c];
    const double kc = a.kc ? a.kc[c] : 0., sc = a.sc ? a.sc[c] : 0.;
    bad[0] += (av >= 0. && av / a.dv < HUGE_VAL) ? 0u : 1u;
    bad[1] += (bv >= 0. && bv < HUGE_VAL) ? 0u : 1u;
    bad[2] += (kc >= 0. && kc < HUGE_VAL) ? 0u : 1u;
    bad[3] += (fabs(sl) < HUGE_VAL) ? 0u : 1u;
    bad[4] += (fabs(sc) < HUGE_VAL && fabs(sl - sc) < HUGE_VAL) ? 0u : 1u;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    for (int off = 32; off > 0; off >>= 1)
      bad[k] += __shfl_down(bad[k], off, 64);
    if (threadIdx.x % 64 == 0 && bad[k])
      atomicAdd(ninvalid + k, bad[k]);
  }
}

struct AbsorbingMarchArgs {
  GridDev grid;
  LineViewDev view;
  const double *records; /* [ncell][6] */
  /* sample rows [sx0, sx1) of the sample grid, as in LineMarchArgs */
  int32_t sx0, sx1;
  /* channels [c0, c0 + nc) of nchan, nc <= CB */
  int32_t c0, nc;
  int32_t full; /* != 0: no window skip */
  int32_t pad;
  double vmin, dv;
  /* sample (sx, sy) of channel c0 + i goes to
   * out[i * channel_stride + (sx - sx0) * ny s + sy] */
  int64_t channel_stride;
  double *out;
  double background[CMI_ABSORBING_MAX_CB]; /* of the block's channels */
};

/* the march of one block of CB channels: one lane per sample ray, far side to
 * near side */
template <int CB, bool CALL>
__global__ void __launch_bounds__(256)
    absorbing_cube_march_kernel(const AbsorbingMarchArgs a) {
  int32_t sx, sy;
  double x, y;
  if (!tile_sample(a.view, a.sx0, a.sx1, sx, sy, x, y))
    return;

  double edge[CB + 1];
  channel_block_edges<CB>(a.vmin, a.dv, a.c0, a.nc, edge);

  double I[CB];
#pragma unroll
  for (int i = 0; i < CB; ++i)
    I[i] = a.background[i];
  double unused = 1.;
  GridRay ray;
  if (ray.start(a.grid, a.view, x, y)) {
    while (ray.inside(a.grid)) {
      const double2 *rec =
          reinterpret_cast<const double2 *>(a.records) + ray.cell(a.grid) * 3;
      const double2 au = rec[0];
      const double2 bs = rec[1];
      const double2 ks = rec[2];
      const double ds = ray.step(a.grid);
      const double adv = au.x, u = au.y, b = bs.x, sl = bs.y;
      const double kc = ks.x, sc = ks.y;
      const double z_lo = (edge[0] - u) / b;
      const double z_hi = (edge[CB] - u) / b;
      const bool dark = !a.full && channel_block_dark(z_lo, z_hi);
      if (dark) {
        if (kc != 0.) {
          const double S = sc + 0. * (sl - sc);
          const double em = absorbing_expm1<CALL>(-(kc * ds));
#pragma unroll
          for (int i = 0; i < CB; ++i)
            absorbing_apply<false>(em, S, I[i], unused);
        }
      } else {
        double E_lo = cube_E(z_lo);
#pragma unroll
        for (int i = 0; i < CB; ++i) {
          const double E_hi = cube_E((edge[i + 1] - u) / b);
          absorbing_channel<false, CALL>(adv, 0.5 * (E_hi - E_lo), sl, kc, sc,
                                         ds, I[i], unused);
          E_lo = E_hi;
        }
      }
    }
  }
  const int64_t at = tile_sample_at(a.view, a.sx0, sx, sy);
#pragma unroll
  for (int i = 0; i < CB; ++i)
    if (i < a.nc)
      a.out[i * a.channel_stride + at] = I[i];
}

struct AbsorbingSkyMarchArgs {
  GridDev grid;
  double origin[3];
  const double *directions; /* [nrays][3] */
  const double *records;    /* [ncell][8] */
  int64_t nrays;
  /* channels [c0, c0 + nc) of nchan, nc <= CB */
  int32_t c0, nc;
  int32_t full; /* != 0: no window skip */
  int32_t pad;
  double vmin, dv;
  /* ray r of channel c0 + i goes to out[(c0 + i) * channel_stride + r] */
  int64_t channel_stride;
  double *out;
  double background[CMI_ABSORBING_MAX_CB]; /* of the block's channels */
};

/* the march of one block of CB channels: one lane per ray, observer
 * outwards. (Named after continuum_sky_march_kernel and not
 * "absorbing_sky_cube_..." on purpose: tests/test_sky_cube_host.py finds the
 * sky cubes' kernel in the listing by the substring sky_cube_march_kernel and
 * expects exactly one. The figures of this kernel are held by
 * tests/test_absorbing_cube_host.py.) */
template <int CB, bool CALL>
__global__ void __launch_bounds__(256)
    absorbing_sky_march_kernel(const AbsorbingSkyMarchArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nrays)
    return;
  double edge[CB + 1];
  channel_block_edges<CB>(a.vmin, a.dv, a.c0, a.nc, edge);

  double I[CB], T[CB];
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    I[i] = 0.;
    T[i] = 1.;
  }
  GridRay ray;
  if (ray.start(a.grid, a.origin, a.directions, r)) {
    while (ray.inside(a.grid)) {
      const double2 *rec =
          reinterpret_cast<const double2 *>(a.records) + ray.cell(a.grid) * 4;
      const double2 aw = rec[0];
      const double2 ww = rec[1];
      const double2 bs = rec[2];
      const double2 ks = rec[3];
      const double ds = ray.step(a.grid);
      const double adv = aw.x, b = bs.x, sl = bs.y, kc = ks.x, sc = ks.y;
      const double u = (aw.y * ray.d[0] + ww.x * ray.d[1]) + ww.y * ray.d[2];
      const double z_lo = (edge[0] - u) / b;
      const double z_hi = (edge[CB] - u) / b;
      const bool dark = !a.full && channel_block_dark(z_lo, z_hi);
      if (dark) {
        if (kc != 0.) {
          const double S = sc + 0. * (sl - sc);
          const double em = absorbing_expm1<CALL>(-(kc * ds));
#pragma unroll
          for (int i = 0; i < CB; ++i)
            absorbing_apply<true>(em, S, I[i], T[i]);
        }
      } else {
        double E_lo = cube_E(z_lo);
#pragma unroll
        for (int i = 0; i < CB; ++i) {
          const double E_hi = cube_E((edge[i + 1] - u) / b);
          absorbing_channel<true, CALL>(adv, 0.5 * (E_hi - E_lo), sl, kc, sc,
                                        ds, I[i], T[i]);
          E_lo = E_hi;
        }
      }
    }
  }
  double *out = a.out + a.c0 * a.channel_stride + r;
#pragma unroll
  for (int i = 0; i < CB; ++i)
    if (i < a.nc)
      out[i * a.channel_stride] = I[i] + T[i] * a.background[i];
}

/* row k of absorbing_cube_probe_kernel with the camera chosen */
template <bool POINT>
__device__ __forceinline__ void absorbing_probe_row(
    const GridDev &g, const LineViewDev &v, const double origin[3],
    const double *__restrict__ rays, int64_t k,
    const double *__restrict__ records, const double *__restrict__ background,
    int32_t nchan, double vmin, double dv, int32_t max_cells, double *o) {
  double *I_steps = o + 3 + 2 * (int64_t)max_cells;
  double *I_end = I_steps + (int64_t)nchan * max_cells;
  for (int32_t c = 0; c < nchan; ++c) {
    const double bg = background[c];
    const double e_lo = vmin + (double)c * dv;
    const double e_hi = vmin + (double)(c + 1) * dv;
    GridRay ray;
    const bool hit = POINT ? ray.start(g, origin, rays, k)
                           : ray.start(g, v, rays[2 * k], rays[2 * k + 1]);
    double I = POINT ? 0. : bg, T = 1.;
    /* (the geometry is every channel's: each writes the same prefix) */
    probe_row(g, ray, hit, max_cells, o, [&](int64_t cell, double ds, int i) {
      const double2 *rec =
          reinterpret_cast<const double2 *>(records) + cell * (POINT ? 4 : 3);
      const double2 r0 = rec[0];
      double u = r0.y;
      if (POINT) {
        const double2 ww = rec[1];
        u = (r0.y * ray.d[0] + ww.x * ray.d[1]) + ww.y * ray.d[2];
      }
      const double2 bs = rec[POINT ? 2 : 1];
      const double2 ks = rec[POINT ? 3 : 2];
      const double f =
          0.5 * (cube_E((e_hi - u) / bs.x) - cube_E((e_lo - u) / bs.x));
      absorbing_channel<POINT, true>(r0.x, f, bs.y, ks.x, ks.y, ds, I, T);
      if (i < max_cells)
        I_steps[(int64_t)c * max_cells + i] = I;
    });
    I_end[c] = POINT ? I + T * bg : I;
  }
}

/* cmi_gpu_absorbing_cube_probe: row k = {t0, t1, steps, cells[max_cells],
 * ds[max_cells], I[nchan][max_cells], I_end[nchan]} of ray k, in the style of
 * continuum_probe_kernel: one channel at a time with the full update in every
 * cell, the march kernels' arithmetic operation for operation. records are
 * the march kernels' (point == 0: 6 doubles per cell, rays[k] = {x, y};
 * otherwise 8, rays from o, rays[k] = the direction); background is [nchan]
 * on the device. */
__global__ void __launch_bounds__(64)
    absorbing_cube_probe_kernel(GridDev g, LineViewDev v, int32_t point,
                                double ox, double oy, double oz,
                                const double *__restrict__ rays, int64_t n,
                                const double *__restrict__ records,
                                const double *__restrict__ background,
                                int32_t nchan, double vmin, double dv,
                                int32_t max_cells, double *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  double *o = out + k * (3 + (2 + (int64_t)nchan) * max_cells + nchan);
  const double origin[3] = {ox, oy, oz};
  if (point)
    absorbing_probe_row<true>(g, v, origin, rays, k, records, background,
                              nchan, vmin, dv, max_cells, o);
  else
    absorbing_probe_row<false>(g, v, origin, rays, k, records, background,
                               nchan, vmin, dv, max_cells, o);
}

#endif
