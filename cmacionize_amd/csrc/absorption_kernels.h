/*
 * absorption_kernels.h - absorption-line spectra: the Voigt optical depth of
 * K resonance lines along sightlines of finite length (include/cmi_gpu.h,
 * "absorption spectra", has the contract; DESIGN.md 4.19 the reasoning and
 * the figures). The absorbing cubes (absorbing_cube_kernels.h) have a
 * Gaussian opacity, one line per call, rays from one origin to the edge of
 * the box and one lane per ray; here a line has damping wings, every ray its
 * own origin and length, and the workload is tens to thousands of rays of a
 * thousand channels, so the mapping is the opposite one.
 *
 * Sightline r: o_r + t d_r, 0 <= t <= L_r, clipped as the point camera's
 * rays are (GridRay::start: t_start, t_out) and walked by GridRay::step. t is
 * the running sum of the path lengths, from t_start. L_r >= t_out (+inf is
 * that) means "to the edge of the box": nothing is cut, the (cell, ds) list
 * is sky_probe's. Otherwise the crossing with t + ds >= L_r has ds = L_r - t
 * and is the last. L_r <= t_start, or a ray that misses: nothing.
 *
 * Per crossing of length ds of a cell with n != 0 (n == 0: nothing at all),
 * u = (w_x d_x + w_y d_y) + w_z d_z with w = v - v_obs, in this order:
 *   nds = n * ds;  N = N + nds;  A = nds * S
 *   f_c = 0.5 * (E((e_{c+1} - u) / b) - E((e_c - u) / b))         (cube_E)
 *   g == 0:  tau_c = tau_c + A * (f_c / dv)
 *   g > 0:   a = g / b;  x = (centre_c - u) / b;  wing = Q(a, x * x) / b
 *            tau_c = tau_c + A * (f_c / dv + wing)
 * e_c = vmin + c * dv, centre_c = 0.5 * (e_c + e_{c+1}); Q is the wing term
 * of lya_voigt (lya_voigt_wing).
 *
 * Records: {w_x, w_y, w_z, 0} per cell and {n, b} per line and cell, fp64,
 * loaded as double2.
 *
 * Mapping: one wave per (ray, line, slab of 64 R consecutive channels), four
 * waves per workgroup with the slab index fastest, so that the waves of a
 * workgroup walk the same ray. Lane j owns the channels c0 + j + 64 i, i < R:
 * the few channels inside a cell's +-6 b window lie on neighbouring lanes.
 * The R accumulators are registers; no atomics, no LDS, no read-modify-write
 * of memory. All lanes walk the same ray and load the same records. With
 * SHARE a lane evaluates E at its lower edges only and takes the upper edge
 * from lane j + 1 (lane 63 from lane 0 of row i + 1; the edge above the slab
 * is lane 0's extra evaluation, for which every other lane passes -inf and
 * leaves cube_E at once): cube_E sees the bits it would see without, so the
 * result is the same. Skips, both wave-uniform and exact: a cell whose window
 * misses the slab (channel_block_dark of the slab's outer edges: every f_c ==
 * 0) is left out with g == 0 and adds A * wing with g > 0, which is
 * A * (0 / dv + wing) bit for bit. full != 0 turns them off.
 */
#ifndef CMI_ABSORPTION_KERNELS_H
#define CMI_ABSORPTION_KERNELS_H

#include "lyman_alpha_kernels.h"
#include "sky_cube_kernels.h"

#define CMI_ABSORPTION_MAX_LINES 16
#define CMI_ABSORPTION_PROBE_CHANNELS 8
/* slab rows per wave (1, 2 or 4) of an axis of more than 128 channels; a
 * shorter axis takes the smallest of 1, 2 and 4 whose slab holds it. The
 * tuning key absorption_slab_rows sets another (0: this rule; DESIGN.md 4.19
 * has the measurement) */
#ifndef CMI_ABSORPTION_R
#define CMI_ABSORPTION_R 4
#endif
/* the tuning key absorption_edge_sharing */
#ifndef CMI_ABSORPTION_EDGE_SHARING
#define CMI_ABSORPTION_EDGE_SHARING 1
#endif

/* the element of each tracked ion as an index into ModelDev::abundance
 * (He C N O Ne S); -1: hydrogen, abundance 1 */
static const int cmi_absorption_ion_element[CMI_NION] = {
    -1, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5, 5};

/* {w, 0} of every cell: w = v - v_obs */
__global__ void __launch_bounds__(256)
    absorption_velocity_record_kernel(const double *__restrict__ velocity,
                                      double vo0, double vo1, double vo2,
                                      int64_t ncell, double *records) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell)
    return;
  const double v_obs[3] = {vo0, vo1, vo2};
  double w[3];
  sky_cube_relative_velocity(velocity, ncell, c, v_obs, w);
  double2 *dst = reinterpret_cast<double2 *>(records) + c * 2;
  dst[0] = make_double2(w[0], w[1]);
  dst[1] = make_double2(w[2], 0.);
}

/* {n, b}[K][ncell] from the caller's n[K][ncell] and b[K][ncell] */
__global__ void __launch_bounds__(256)
    field_absorption_record_kernel(const double *__restrict__ n,
                                   const double *__restrict__ b, int64_t count,
                                   double2 *records) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count)
    records[i] = make_double2(n[i], b[i]);
}

struct AbsorptionIonRecordArgs {
  CellsDev cells;
  int64_t ncell;
  int32_t nlines;
  int32_t ion[CMI_ABSORPTION_MAX_LINES];
  double abundance[CMI_ABSORPTION_MAX_LINES]; /* of the ion's element */
  double weight[CMI_ABSORPTION_MAX_LINES];    /* its atomic weight */
  double sigma_turb;
  double2 *records;
};

/* {n, b}[K][ncell] from the cells as they are: n = n_H A x_ion,
 * b = sqrt(2 k T / (w m_u) + 2 sigma_turb^2) */
__global__ void __launch_bounds__(256)
    absorption_ion_record_kernel(const AbsorptionIonRecordArgs a) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.ncell)
    return;
  const double n_H = a.cells.number_density[c];
  const double T = a.cells.temperature[c];
  for (int l = 0; l < a.nlines; ++l) {
    const double n = n_H * a.abundance[l] * a.cells.x[a.ion[l]][c];
    const double thermal =
        (T > 0.) ? 2. * CMI_BOLTZMANN * T / (a.weight[l] * CMI_ATOMIC_MASS_UNIT)
                 : 0.;
    const double b = sqrt(thermal + 2. * a.sigma_turb * a.sigma_turb);
    a.records[(int64_t)l * a.ncell + c] = make_double2(n, b);
  }
}

/* what the contract refuses in records {n, b}[K][ncell], added to
 * ninvalid[0 .. 2]: n negative or not finite; b negative or not finite; a
 * cell with n > 0 and b == 0 of a line with g > 0 (one atomic per wave and
 * count that found any) */
__global__ void __launch_bounds__(256)
    absorption_record_check_kernel(const double2 *__restrict__ records,
                                   const double *__restrict__ g, int64_t ncell,
                                   int32_t nlines, unsigned int *ninvalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad[3] = {0, 0, 0};
  for (int l = 0; l < nlines; ++l) {
    const double gl = g[l];
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell;
         c += stride) {
      const double2 nb = records[(int64_t)l * ncell + c];
      bad[0] += (nb.x >= 0. && nb.x < HUGE_VAL) ? 0u : 1u;
      bad[1] += (nb.y >= 0. && nb.y < HUGE_VAL) ? 0u : 1u;
      bad[2] += (nb.x > 0. && gl > 0. && nb.y == 0.) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1)
      bad[k] += __shfl_down(bad[k], off, 64);
    if (threadIdx.x % 64 == 0 && bad[k])
      atomicAdd(ninvalid + k, bad[k]);
  }
}

/* a sightline's walk: the point camera's ray and the contract's cut */
struct AbsorptionWalk {
  GridRay ray;
  double t, cut;
  bool more;

  __device__ __forceinline__ bool start(const GridDev &g,
                                        const double *__restrict__ origins,
                                        const double *__restrict__ directions,
                                        const double *__restrict__ lengths,
                                        int64_t r, bool &hit) {
    const double o[3] = {origins[3 * r], origins[3 * r + 1],
                         origins[3 * r + 2]};
    const double L = lengths[r];
    hit = ray.start(g, o, directions, r);
    more = hit && L > ray.t0;
    t = ray.t0;
    cut = (L < ray.t1) ? L : HUGE_VAL;
    return more;
  }

  __device__ __forceinline__ bool inside(const GridDev &g) const {
    return more && ray.inside(g);
  }

  /* the path length in the cell the ray is in, cut at L */
  __device__ __forceinline__ double step(const GridDev &g) {
    double ds = ray.step(g);
    if (t + ds >= cut) {
      ds = cut - t;
      more = false;
    }
    t = t + ds;
    return ds;
  }
};

/* the contract's update of one channel */
__device__ __forceinline__ double absorption_wing(double g, double b,
                                                  double centre, double u) {
  const double x = (centre - u) / b;
  return lya_voigt_wing(g / b, x * x) / b;
}

/* lane j + 1's value for lane j, lane 63 keeps its own: a wavefront shift by
 * one lane (DPP wave_shl:1 on either half; __shfl_down(v, 1) compiles to two
 * ds_bpermute_b32 with their address arithmetic instead) */
__device__ __forceinline__ double absorption_next_lane(double v) {
  union {
    double d;
    int i[2];
  } in, out;
  in.d = v;
  out.i[0] = __builtin_amdgcn_update_dpp(in.i[0], in.i[0], 0x130, 0xf, 0xf,
                                         false);
  out.i[1] = __builtin_amdgcn_update_dpp(in.i[1], in.i[1], 0x130, 0xf, 0xf,
                                         false);
  return out.d;
}

/* lane 0's value for every lane */
__device__ __forceinline__ double absorption_lane_zero(double v) {
  union {
    double d;
    int i[2];
  } in, out;
  in.d = v;
  out.i[0] = __builtin_amdgcn_readlane(in.i[0], 0);
  out.i[1] = __builtin_amdgcn_readlane(in.i[1], 0);
  return out.d;
}

struct AbsorptionMarchArgs {
  GridDev grid;
  const double *origins, *directions, *lengths; /* [nrays][3], [3], [1] */
  const double *velocity_records;               /* [ncell][4] */
  const double2 *records;                       /* [K][ncell] {n, b} */
  const double *S, *g;                          /* [K] */
  int64_t ncell;
  uint32_t nitems; /* nrays K nslab */
  uint32_t nlines, nslab;
  int32_t nchan;
  int32_t full; /* != 0: no skips */
  int32_t pad;
  double vmin, dv;
  double *tau; /* [nrays][K][nchan] */
  double *N;   /* [nrays][K] */
};

template <int R, bool SHARE>
__global__ void __launch_bounds__(256)
    absorption_march_kernel(const AbsorptionMarchArgs a) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t lane = threadIdx.x & 63;
  const uint32_t item = blockIdx.x * 4u + wave;
  if (item >= a.nitems)
    return;
  const uint32_t slab = item % a.nslab;
  const uint32_t rl = item / a.nslab;
  const uint32_t line = rl % a.nlines;
  const int64_t r = rl / a.nlines;
  const int32_t c0 = (int32_t)slab * (64 * R);

  double e_lo[R], e_hi[R], centre[R], tau[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int32_t c = c0 + lane + 64 * i;
    e_lo[i] = a.vmin + (double)c * a.dv;
    e_hi[i] = a.vmin + (double)(c + 1) * a.dv;
    centre[i] = 0.5 * (e_lo[i] + e_hi[i]);
    tau[i] = 0.;
  }
  const double slab_lo = a.vmin + (double)c0 * a.dv;
  const double slab_hi = a.vmin + (double)(c0 + 64 * R) * a.dv;
  const double S = a.S[line], g = a.g[line];
  const double2 *records = a.records + (int64_t)line * a.ncell;
  double N = 0.;

  AbsorptionWalk walk;
  bool hit;
  if (walk.start(a.grid, a.origins, a.directions, a.lengths, r, hit)) {
    const double *d = walk.ray.d;
    while (walk.inside(a.grid)) {
      const int64_t cell = walk.ray.cell(a.grid);
      const double2 nb = records[cell];
      const double2 *wrec =
          reinterpret_cast<const double2 *>(a.velocity_records) + cell * 2;
      const double2 w01 = wrec[0];
      const double2 w2 = wrec[1];
      const double ds = walk.step(a.grid);
      const double n = nb.x, b = nb.y;
      if (n == 0.)
        continue;
      const double nds = n * ds;
      N = N + nds;
#ifdef CMI_ABSORPTION_WALK_ONLY
      /* (experiments build: the walk and the record loads without the
       * deposit) */
      tau[0] = tau[0] + nds * w2.x;
      continue;
#endif
      const double A = nds * S;
      const double u = (w01.x * d[0] + w01.y * d[1]) + w2.x * d[2];
      const bool dark =
          !a.full && channel_block_dark((slab_lo - u) / b, (slab_hi - u) / b);
      if (dark) {
        if (g != 0.) {
#pragma unroll
          for (int i = 0; i < R; ++i)
            tau[i] = tau[i] + A * absorption_wing(g, b, centre[i], u);
        }
        continue;
      }
      double E[R + 1];
#pragma unroll
      for (int i = 0; i < R; ++i)
        E[i] = cube_E((e_lo[i] - u) / b);
      if (SHARE)
        E[R] = cube_E(lane == 0 ? (slab_hi - u) / b : -HUGE_VAL);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        double E_hi;
        if (SHARE) {
          const double next = absorption_next_lane(E[i]);
          const double wrap = absorption_lane_zero(E[i + 1]);
          E_hi = (lane == 63) ? wrap : next;
        } else {
          E_hi = cube_E((e_hi[i] - u) / b);
        }
        const double core = 0.5 * (E_hi - E[i]) / a.dv;
        if (g != 0.)
          tau[i] = tau[i] + A * (core + absorption_wing(g, b, centre[i], u));
        else
          tau[i] = tau[i] + A * core;
      }
    }
  }
  double *out = a.tau + ((int64_t)rl * a.nchan + c0);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int32_t c = lane + 64 * i;
    if (c0 + c < a.nchan)
      out[c] = tau[i];
  }
  if (slab == 0 && lane == 0)
    a.N[rl] = N;
}

/* cmi_gpu_absorption_probe: the row {t0, t1, steps, cells[max_cells],
 * ds[max_cells], tau[nc][max_cells], tau_end[nc]} of one ray and one line
 * for the nc <= 8 channels `channels`: the march kernel's arithmetic
 * operation for operation, one channel at a time, without skips. A ray that
 * misses has {NaN, NaN, 0}. One thread. */
__global__ void __launch_bounds__(64)
    absorption_probe_kernel(GridDev grid, const double *__restrict__ ray,
                            const double *__restrict__ velocity_records,
                            const double2 *__restrict__ records, double S,
                            double g, const int32_t *__restrict__ channels,
                            int32_t nc, double vmin, double dv,
                            int32_t max_cells, double *__restrict__ o) {
  if (blockIdx.x != 0 || threadIdx.x != 0)
    return;
  double *tau_steps = o + 3 + 2 * (int64_t)max_cells;
  double *tau_end = tau_steps + (int64_t)nc * max_cells;
  for (int32_t k = 0; k < (nc > 0 ? nc : 1); ++k) {
    const int32_t c = nc > 0 ? channels[k] : 0;
    const double e_lo = vmin + (double)c * dv;
    const double e_hi = vmin + (double)(c + 1) * dv;
    const double centre = 0.5 * (e_lo + e_hi);
    AbsorptionWalk walk;
    bool hit;
    double tau = 0.;
    int steps = 0;
    /* (the geometry is every channel's: each writes the same prefix) */
    walk.start(grid, ray, ray + 3, ray + 6, 0, hit);
    while (walk.inside(grid)) {
      const int64_t cell = walk.ray.cell(grid);
      const double2 nb = records[cell];
      const double2 *wrec =
          reinterpret_cast<const double2 *>(velocity_records) + cell * 2;
      const double2 w01 = wrec[0];
      const double2 w2 = wrec[1];
      const double ds = walk.step(grid);
      const double n = nb.x, b = nb.y;
      if (n != 0.) {
        const double nds = n * ds;
        const double A = nds * S;
        const double u = (w01.x * walk.ray.d[0] + w01.y * walk.ray.d[1]) +
                         w2.x * walk.ray.d[2];
        const double core =
            0.5 * (cube_E((e_hi - u) / b) - cube_E((e_lo - u) / b)) / dv;
        if (g != 0.)
          tau = tau + A * (core + absorption_wing(g, b, centre, u));
        else
          tau = tau + A * core;
      }
      if (steps < max_cells) {
        o[3 + steps] = (double)cell;
        o[3 + max_cells + steps] = ds;
        if (nc > 0)
          tau_steps[(int64_t)k * max_cells + steps] = tau;
      }
      ++steps;
    }
    o[0] = hit ? walk.ray.t0 : __builtin_nan("");
    o[1] = hit ? walk.ray.t1 : __builtin_nan("");
    o[2] = (double)steps;
    if (nc > 0)
      tau_end[k] = tau;
  }
}

#endif
