/*
 * dust_kernels.h - kernels of the dusty radiative transfer mode: one thread
 * per packet of DustPhotonShootJob::execute
 * (src/DustPhotonShootJob.hpp:107-164). Both marches (interact up to an
 * optical depth, integrate_optical_depth to the box edge) are dda_step over
 * the per-cell records {n kappa x_H, 0} built by dust_opacity_kernel; the
 * peel-off I, Q, U go into the image with fp64 atomics.
 */
#ifndef CMI_DUST_KERNELS_H
#define CMI_DUST_KERNELS_H

#include "device_dust.h"

/* {n kappa x_H, 0} per cell (the march reads .x; .y is multiplied by
 * sigma_He_corr = 0) */
__global__ void __launch_bounds__(256)
    dust_opacity_kernel(const double *__restrict__ number_density,
                        const double *__restrict__ xH, double kappa,
                        int64_t ncell, double2 *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncell)
    out[i] = make_double2(number_density[i] * kappa * xH[i], 0.);
}

/* {n sigma, 0} per cell: dust that follows the gas, sigma per hydrogen
 * nucleus (cmi_gpu_set_dust_scattering_per_hydrogen); x_H is not read */
__global__ void __launch_bounds__(256)
    dust_opacity_per_hydrogen_kernel(const double *__restrict__ number_density,
                                     double sigma, int64_t ncell,
                                     double2 *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncell)
    out[i] = make_double2(number_density[i] * sigma, 0.);
}

/* what one packet contributes to the image: either atomics into d.image
 * (TRACE = false) or the event rows {x, y, z, I, Q, U, V, weight} of a trace
 * (the direct light first, then one row per scattering) */
struct DustEvents {
  double *rows;
  int max_events;
  int n;
};

/* the next row of a trace: {x, y, z, I, Q, U, V, weight} and what the caller
 * appends (`more`: the cube run's u and b); beyond max_events the event is
 * counted and no row is written */
template <class... MORE>
__device__ __forceinline__ void
dust_trace_row(DustEvents &ev, const double pos[3], const double stokes[4],
               double weight, MORE... more) {
  if (ev.n < ev.max_events) {
    double *r = ev.rows + (int)(8 + sizeof...(MORE)) * ev.n;
    r[0] = pos[0];
    r[1] = pos[1];
    r[2] = pos[2];
    r[3] = stokes[0];
    r[4] = stokes[1];
    r[5] = stokes[2];
    r[6] = stokes[3];
    r[7] = weight;
    [[maybe_unused]] int j = 8;
    ((r[j++] = more), ...);
  }
  ++ev.n;
}

template <bool TRACE>
__device__ __forceinline__ void dust_add(const DustDev &d, const double pos[3],
                                         double wi, double wq, double wu,
                                         const double stokes[4], double weight,
                                         DustEvents &ev,
                                         unsigned long long &natomics) {
  if (TRACE) {
    dust_trace_row(ev, pos, stokes, weight);
    return;
  }
  const int64_t pixel = dust_pixel(d, pos);
  if (pixel < 0)
    return;
  const int64_t npixel = (int64_t)d.res[0] * d.res[1];
  /* x + 0 == x: zero terms (Q and U of the direct light, a packet on a ray
   * without dust) cost no atomic */
  if (wi != 0.) {
    atomicAdd(d.image + pixel, wi);
    ++natomics;
  }
  if (wq != 0.) {
    atomicAdd(d.image + npixel + pixel, wq);
    ++natomics;
  }
  if (wu != 0.) {
    atomicAdd(d.image + 2 * npixel + pixel, wu);
    ++natomics;
  }
}

/* the point camera's dust_add: I, Q, U into pixel `pixel` of cam.image (-1:
 * outside the window, counted), or the trace's row */
template <bool TRACE>
__device__ __forceinline__ void
dust_sky_add(const SkyCameraDev &cam, const double pos[3], int64_t pixel,
             double wi, double wq, double wu, const double stokes[4],
             double weight, DustEvents &ev, DustCountersDev &c) {
  if (TRACE) {
    dust_trace_row(ev, pos, stokes, weight);
    return;
  }
  if (pixel < 0) {
    c.noutside += 1;
    return;
  }
  const int64_t npixel = (int64_t)cam.nlon * cam.nlat;
  if (wi != 0.) {
    atomicAdd(cam.image + pixel, wi);
    ++c.natomics;
  }
  if (wq != 0.) {
    atomicAdd(cam.image + npixel + pixel, wq);
    ++c.natomics;
  }
  if (wu != 0.) {
    atomicAdd(cam.image + 2 * npixel + pixel, wu);
    ++c.natomics;
  }
}

/* one event of the point camera (device_dust.h's header comment has the
 * contract): the direct light of the photon at its emission point (`scattered`
 * false, w = 1) or the peel-off of a copy of it at a scattering point
 * (w = the packet's weight so far, albedo included). An event inside the
 * exclusion radius is counted and adds nothing (a trace gets a row of zeros
 * at its position: one row per event, as with the parallel camera).
 * __noinline__ like the functions it calls: one copy serves
 * the direct light and the peel-offs. */
template <bool TRACE>
__device__ __noinline__ void
dust_sky_event(const GridDev &g, const DustDev &d, const SkyCameraDev &cam,
               const double2 *__restrict__ opacity, DustPhoton &peel,
               bool scattered, double weight, double albedo,
               DustCountersDev &c, DustEvents &ev) {
  double k[3], r, r2;
  if (!dust_sky_direction(cam, peel.pos, k, r, r2)) {
    c.nexcluded += 1;
    const double nothing[4] = {0., 0., 0., 0.};
    if (TRACE)
      dust_sky_add<TRACE>(cam, peel.pos, -1, 0., 0., 0., nothing, 0., ev, c);
    return;
  }
  double w;
  if (scattered) {
    const double hgfac = dust_scatter_towards_point(d, peel, k);
    const double tau = dust_integrate_to(g, opacity, peel.pos, peel.dir,
                                         peel.inv_dir, r, c.nsteps);
    if (!cam.pole_is_z)
      dust_sky_rotate(cam, k, peel.stokes);
    w = weight * hgfac * albedo * exp(-tau);
  } else {
    const double inv_k[3] = {1. / k[0], 1. / k[1], 1. / k[2]};
    const double tau =
        dust_integrate_to(g, opacity, peel.pos, k, inv_k, r, c.nsteps);
    w = 0.25 * exp(-tau) / M_PI;
  }
  const double addend = w / r2;
  const int64_t pixel = TRACE ? -1 : dust_sky_pixel(cam, k);
  dust_sky_add<TRACE>(cam, peel.pos, pixel, addend * peel.stokes[0],
                      addend * peel.stokes[1], addend * peel.stokes[2],
                      peel.stokes, addend, ev, c);
}

/* what one view's event added to the thread's counters since `before`, into
 * the view's own (device_dust.h has the layout) */
__device__ __forceinline__ void dust_view_count(unsigned long long *counters,
                                                int v,
                                                const DustCountersDev &before,
                                                const DustCountersDev &c) {
  unsigned long long *dst =
      counters +
      (size_t)v * CMI_DUST_VIEW_COUNTERS * CMI_DUST_VIEW_SLOTS +
      threadIdx.x % CMI_DUST_VIEW_SLOTS;
  const unsigned long long delta[CMI_DUST_VIEW_COUNTERS] = {
      c.nsteps - before.nsteps, c.natomics - before.natomics,
      c.nexcluded - before.nexcluded, c.noutside - before.noutside};
#pragma unroll
  for (int j = 0; j < CMI_DUST_VIEW_COUNTERS; ++j)
    if (delta[j])
      atomicAdd(dst + j * CMI_DUST_VIEW_SLOTS, delta[j]);
}

/* view v of the parallel views as the single camera's DustDev: dv is a copy
 * of the kernel's d, of which only the camera's fields change */
__device__ __forceinline__ void
dust_select_view(const DustCamera<DUST_CAMERA_PARALLEL_VIEWS> &cam, int v,
                 DustDev &dv) {
  const DustViewDev &w = cam.views[v];
#pragma unroll
  for (int j = 0; j < 5; ++j)
    dv.view[j] = w.view[j];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    dv.obs_dir[a] = w.obs_dir[a];
    dv.obs_inv_dir[a] = w.obs_inv_dir[a];
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    dv.img_anchor[a] = w.img_anchor[a];
    dv.img_sides[a] = w.img_sides[a];
  }
  dv.image = cam.images + (size_t)v * 3 * ((size_t)dv.res[0] * dv.res[1]);
}

/* observer v of the point views as the single camera's SkyCameraDev: cv is a
 * copy of cam.shared */
__device__ __forceinline__ void
dust_select_view(const DustCamera<DUST_CAMERA_POINT_VIEWS> &cam, int v,
                 SkyCameraDev &cv) {
  const SkyObserverDev &w = cam.views[v];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cv.o[a] = w.o[a];
    cv.e1[a] = w.e1[a];
    cv.e2[a] = w.e2[a];
    cv.e3[a] = w.e3[a];
  }
  cv.r_min2 = w.r_min2;
  cv.pole_is_z = w.pole_is_z;
  cv.image = cam.images + (size_t)v * 3 * ((size_t)cv.nlon * cv.nlat);
}

/* Cube mode (scattered-light line cubes; include/cmi_gpu.h,
 * "scattered-light line cubes", has the contract): the compile-time switch
 * CUBE of dust_packet and its kernels, and what a cube run reads beyond the
 * image run, a kernel argument of its own. Only the cell source has it. The
 * events of a cube run are dust_cube_kernels.h's. */
template <bool CUBE> struct DustCube {};
template <> struct DustCube<true> {
  const double *velocity;     /* [3][ncell] or null: at rest */
  int64_t ncell;
  const double *s2;           /* [ncell]: the variance of a cell's profile */
  const double *obs_velocity; /* [nviews][3]; the point camera's */
  double two_sigma2;          /* 2 sigma_t sigma_t */
  int32_t nchan;
  double vmin, dv;
  int64_t npixel; /* of one view's image */
  double *cube;   /* [nviews][3][npixel][nchan]: the channel runs fastest */
};
typedef DustCube<true> DustCubeDev;

template <bool TRACE, int CAMERA>
__device__ __forceinline__ void
dust_cube_events(const GridDev &g, const DustDev &d,
                 const DustCamera<CAMERA> &cam, const DustCubeDev &cube,
                 const double2 *__restrict__ opacity, const DustPhoton &p,
                 bool scattered, double weight, double albedo, double q,
                 double s2, int64_t cell, DustDev &dv, SkyCameraDev &cv,
                 DustCountersDev &c, DustEvents &ev);
__device__ __forceinline__ double dust_cube_doppler(const DustCubeDev &cube,
                                                    int64_t cell,
                                                    const double k[3]);
__device__ __forceinline__ int64_t dust_cube_cell(const GridDev &g,
                                                  const double pos[3]);

/* DustPhotonShootJob::execute for one packet; SOURCE selects where it
 * starts and CAMERA where its peel-offs go (at compile time: the galaxy's
 * instantiation has no trace of the other source, the parallel camera's
 * none of the point camera), everything else is the same. The two kinds with
 * several views walk the same walk and repeat each event per view, in the
 * order 0..K-1, through the single camera's functions with the single
 * camera's expressions: an addend is the single camera's addend. With CUBE
 * the packet carries its Doppler velocity q and the variance s2 of its
 * profile, and every event goes through dust_cube_events, which fills the
 * image with the same addends and the cube with their shares per channel;
 * the walk and its random numbers do not change. */
template <bool TRACE, int SOURCE, int CAMERA, bool CUBE>
__device__ inline void dust_packet(const GridDev &g, const DustDev &d,
                                   const DustSource<SOURCE> &src,
                                   const DustCamera<CAMERA> &cam,
                                   const DustCube<CUBE> &cube,
                                   const double2 *__restrict__ opacity,
                                   uint32_t seed, uint64_t id,
                                   DustCountersDev &c, DustEvents &ev) {
  PacketRng rng;
  rng.init(seed, 0u, id);
  DustPhoton p;
  c.npackets += 1;
  /* cube mode's two scalars */
  [[maybe_unused]] double q = 0., s2 = 0.;
  [[maybe_unused]] int64_t ecell = 0;
  if constexpr (SOURCE == DUST_SOURCE_CELLS) {
    if constexpr (CUBE) {
      ecell = dust_emit_cells(g, src, rng, p);
      q = dust_cube_doppler(cube, ecell, p.dir);
      s2 = cube.s2[ecell];
    } else {
      (void)dust_emit_cells(g, src, rng, p);
    }
  } else {
    if (!dust_emit(d, rng, p)) {
      c.nsource_capped += 1;
      return;
    }
  }

  /* the single camera that the current view is handed to the camera's
   * functions as (several views only; unused and gone otherwise) */
  DustDev dv;
  SkyCameraDev cv;
  if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS)
    dv = d;
  if constexpr (CAMERA == DUST_CAMERA_POINT_VIEWS)
    cv = cam.shared;

  /* direct light towards the observer, :127-130 */
  if constexpr (CUBE) {
    dust_cube_events<TRACE, CAMERA>(g, d, cam, cube, opacity, p, false, 1., 1.,
                                    q, s2, ecell, dv, cv, c, ev);
  } else if constexpr (CAMERA == DUST_CAMERA_POINT_VIEWS) {
    if (cam.shared.direct_light) {
      for (int v = 0; v < cam.nviews; ++v) {
        dust_select_view(cam, v, cv);
        const DustCountersDev before = c;
        DustPhoton direct = p;
        dust_sky_event<TRACE>(g, d, cv, opacity, direct, false, 1., 1., c, ev);
        dust_view_count(cam.counters, v, before, c);
      }
    }
  } else if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS) {
    for (int v = 0; v < cam.nviews; ++v) {
      dust_select_view(cam, v, dv);
      const DustCountersDev before = c;
      const double tau_old = dust_integrate(g, opacity, p.pos, dv.obs_dir,
                                            dv.obs_inv_dir, c.nsteps);
      const double w_direct = 0.25 * exp(-tau_old) / M_PI;
      const double unpolarised[4] = {1., 0., 0., 0.};
      dust_add<TRACE>(dv, p.pos, w_direct, 0., 0., unpolarised, w_direct, ev,
                      c.natomics);
      dust_view_count(cam.counters, v, before, c);
    }
  } else if constexpr (CAMERA == DUST_CAMERA_POINT) {
    if (cam.direct_light) {
      DustPhoton direct = p;
      dust_sky_event<TRACE>(g, d, cam, opacity, direct, false, 1., 1., c, ev);
    }
  } else {
    const double tau_old =
        dust_integrate(g, opacity, p.pos, d.obs_dir, d.obs_inv_dir, c.nsteps);
    const double w_direct = 0.25 * exp(-tau_old) / M_PI;
    const double unpolarised[4] = {1., 0., 0., 0.};
    dust_add<TRACE>(d, p.pos, w_direct, 0., 0., unpolarised, w_direct, ev,
                    c.natomics);
  }

  /* forced first interaction, :132-138 */
  double albedo = 1.;
  const double tau_max =
      dust_integrate(g, opacity, p.pos, p.dir, p.inv_dir, c.nsteps);
  const double weight = 1. - exp(-tau_max);
  double tau = -log(1. - rng.next() * weight);
  bool inside = dust_interact(g, opacity, p, tau, c.nsteps);
  uint32_t nscatter = 0;
  while (inside) {
    /* peel-off, :141-155 */
    DustPhoton peel = p;
    if constexpr (CUBE) {
      albedo *= d.albedo;
      dust_cube_events<TRACE, CAMERA>(g, d, cam, cube, opacity, p, true,
                                      weight, albedo, q, s2,
                                      dust_cube_cell(g, p.pos), dv, cv, c, ev);
    } else if constexpr (CAMERA == DUST_CAMERA_POINT_VIEWS) {
      albedo *= d.albedo;
      for (int v = 0; v < cam.nviews; ++v) {
        dust_select_view(cam, v, cv);
        const DustCountersDev before = c;
        peel = p;
        dust_sky_event<TRACE>(g, d, cv, opacity, peel, true, weight, albedo, c,
                              ev);
        dust_view_count(cam.counters, v, before, c);
      }
    } else if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS) {
      albedo *= d.albedo;
      for (int v = 0; v < cam.nviews; ++v) {
        dust_select_view(cam, v, dv);
        const DustCountersDev before = c;
        peel = p;
        const double hgfac = dust_scatter_towards(dv, peel);
        const double tau_new = dust_integrate(g, opacity, peel.pos, peel.dir,
                                              peel.inv_dir, c.nsteps);
        const double weight_new = weight * hgfac * albedo * exp(-tau_new);
        dust_add<TRACE>(dv, peel.pos, weight_new * peel.stokes[0],
                        weight_new * peel.stokes[1],
                        weight_new * peel.stokes[2], peel.stokes, weight_new,
                        ev, c.natomics);
        dust_view_count(cam.counters, v, before, c);
      }
    } else if constexpr (CAMERA == DUST_CAMERA_POINT) {
      albedo *= d.albedo;
      dust_sky_event<TRACE>(g, d, cam, opacity, peel, true, weight, albedo, c,
                            ev);
    } else {
      const double hgfac = dust_scatter_towards(d, peel);
      const double tau_new = dust_integrate(g, opacity, peel.pos, peel.dir,
                                            peel.inv_dir, c.nsteps);
      albedo *= d.albedo;
      const double weight_new = weight * hgfac * albedo * exp(-tau_new);
      dust_add<TRACE>(d, peel.pos, weight_new * peel.stokes[0],
                      weight_new * peel.stokes[1], weight_new * peel.stokes[2],
                      peel.stokes, weight_new, ev, c.natomics);
    }
    /* scatter and fly on, :157-159 */
    if constexpr (CUBE) {
      const int64_t scell = dust_cube_cell(g, p.pos);
      const double k[3] = {p.dir[0], p.dir[1], p.dir[2]};
      dust_scatter(d, rng, p);
      q += dust_cube_doppler(cube, scell, p.dir) -
           dust_cube_doppler(cube, scell, k);
      s2 += cube.two_sigma2 *
            fmax(0., 1. - ((k[0] * p.dir[0] + k[1] * p.dir[1]) +
                           k[2] * p.dir[2]));
    } else {
      dust_scatter(d, rng, p);
    }
    ++nscatter;
    if (nscatter >= CMI_DUST_MAX_SCATTER) {
      c.ncapped += 1;
      break;
    }
    tau = -log(rng.next());
    inside = dust_interact(g, opacity, p, tau, c.nsteps);
  }
  c.nscatter += nscatter;
}

/* sum of a 64-bit counter over the wave, added by its first active lane */
__device__ __forceinline__ void dust_count(unsigned long long *dst,
                                           unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off, 64);
  if (threadIdx.x % 64 == 0 && v)
    atomicAdd(dst, v);
}

/* packets [first, first + n) */
template <int SOURCE, int CAMERA, bool CUBE>
__global__ void __launch_bounds__(256)
    dust_shoot_kernel(GridDev g, DustDev d,
                      const double2 *__restrict__ opacity, uint32_t seed,
                      uint64_t first, uint64_t n, DustCountersDev *counters,
                      DustSource<SOURCE> src, DustCamera<CAMERA> cam,
                      DustCube<CUBE> cube) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  DustCountersDev c = {};
  DustEvents ev = {nullptr, 0, 0};
  if (k < n)
    dust_packet<false, SOURCE, CAMERA, CUBE>(g, d, src, cam, cube, opacity,
                                             seed, first + k, c, ev);
  /* the whole wave reaches the reduction (no early return above) */
  dust_count(&counters->nsteps, c.nsteps);
  dust_count(&counters->nscatter, c.nscatter);
  dust_count(&counters->ncapped, c.ncapped);
  dust_count(&counters->natomics, c.natomics);
  dust_count(&counters->npackets, c.npackets);
  dust_count(&counters->nsource_capped, c.nsource_capped);
  if constexpr (CAMERA == DUST_CAMERA_POINT ||
                CAMERA == DUST_CAMERA_POINT_VIEWS) {
    dust_count(&counters->nexcluded, c.nexcluded);
    dust_count(&counters->noutside, c.noutside);
  }
}

enum {
  DUST_PROBE_EMIT = 0,
  DUST_PROBE_SCATTER = 1,
  DUST_PROBE_SCATTER_TOWARDS = 2,
  DUST_PROBE_OPTICAL_DEPTH = 3,
  DUST_PROBE_TRACE = 4,
  DUST_PROBE_CELL_SOURCE = 5,
  DUST_PROBE_SKY_PEEL = 6,
  DUST_PROBE_CUBE_TRACE = 7
};

/* the parity probes of cmi_gpu_dust_probe (include/cmi_gpu.h gives the row
 * layouts); row k uses the stream of packet first + k. EMIT and TRACE follow
 * SOURCE, TRACE follows CAMERA; CELL_SOURCE exists in the cell source's
 * instantiations only, SKY_PEEL in the point camera's. The CUBE
 * instantiations serve CUBE_TRACE alone: TRACE with rows of 10, {u, b} after
 * the 8. */
template <int SOURCE, int CAMERA, bool CUBE>
__global__ void __launch_bounds__(64)
    dust_probe_kernel(GridDev g, DustDev d, DustSource<SOURCE> src,
                      DustCamera<CAMERA> cam, DustCube<CUBE> cube,
                      const double2 *__restrict__ opacity, int32_t kind,
                      uint32_t seed, uint64_t first, int64_t n, int32_t width,
                      const double *__restrict__ in, double *__restrict__ out,
                      int32_t max_events) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  PacketRng rng;
  rng.init(seed, 0u, first + k);
  double *o = out + k * width;
  if constexpr (CUBE) {
    if (kind == DUST_PROBE_CUBE_TRACE) {
      DustCountersDev c = {};
      DustEvents ev = {o + 4, max_events, 0};
      dust_packet<true, SOURCE, CAMERA, true>(g, d, src, cam, cube, opacity,
                                              seed, first + k, c, ev);
      o[0] = ev.n;
      o[1] = (double)c.nscatter;
      o[2] = (double)c.nsteps;
      o[3] = (double)(c.ncapped + c.nsource_capped);
    }
    return;
  }
  if (kind == DUST_PROBE_EMIT) {
    DustPhoton p;
    bool ok = true;
    if constexpr (SOURCE == DUST_SOURCE_CELLS)
      (void)dust_emit_cells(g, src, rng, p);
    else
      ok = dust_emit(d, rng, p);
    for (int a = 0; a < 3; ++a) {
      o[a] = ok ? p.pos[a] : __builtin_nan("");
      o[3 + a] = ok ? p.dir[a] : __builtin_nan("");
    }
  } else if (kind == DUST_PROBE_SCATTER ||
             kind == DUST_PROBE_SCATTER_TOWARDS) {
    /* in: {dir[3], sin theta, cos theta, phi, sin phi, cos phi, I, Q, U, V} */
    const double *r = in + k * 12;
    DustPhoton p;
    dust_set_direction(p, r);
    for (int j = 0; j < 5; ++j)
      p.par[j] = r[3 + j];
    for (int j = 0; j < 4; ++j)
      p.stokes[j] = r[8 + j];
    for (int a = 0; a < 3; ++a)
      p.pos[a] = 0.;
    if (kind == DUST_PROBE_SCATTER) {
      dust_scatter(d, rng, p);
      for (int a = 0; a < 3; ++a)
        o[a] = p.dir[a];
      for (int j = 0; j < 5; ++j)
        o[3 + j] = p.par[j];
      for (int j = 0; j < 4; ++j)
        o[8 + j] = p.stokes[j];
    } else {
      o[0] = dust_scatter_towards(d, p);
      for (int j = 0; j < 4; ++j)
        o[1 + j] = p.stokes[j];
    }
  } else if (kind == DUST_PROBE_OPTICAL_DEPTH) {
    /* in: {pos[3], dir[3]}; out: {tau, nsteps, cells[max_events]} */
    const double *r = in + k * 6;
    double inv[3];
    for (int a = 0; a < 3; ++a)
      inv[a] = 1. / r[3 + a];
    unsigned long long nsteps = 0;
    o[0] = dust_integrate(g, opacity, r, r + 3, inv, nsteps, o + 2,
                          max_events);
    o[1] = (double)nsteps;
  } else if (kind == DUST_PROBE_TRACE) {
    /* out: {nevents, nscatter, nsteps, ncapped, rows[max_events][8]} */
    DustCountersDev c = {};
    DustEvents ev = {o + 4, max_events, 0};
    dust_packet<true, SOURCE, CAMERA, false>(g, d, src, cam, DustCube<false>(),
                                             opacity, seed, first + k, c, ev);
    o[0] = ev.n;
    o[1] = (double)c.nscatter;
    o[2] = (double)c.nsteps;
    o[3] = (double)(c.ncapped + c.nsource_capped);
  } else if (kind == DUST_PROBE_CELL_SOURCE) {
    /* out: {cell, pos[3], dir[3]} */
    if constexpr (SOURCE == DUST_SOURCE_CELLS) {
      DustPhoton p;
      o[0] = (double)dust_emit_cells(g, src, rng, p);
      for (int a = 0; a < 3; ++a) {
        o[1 + a] = p.pos[a];
        o[4 + a] = p.dir[a];
      }
    }
  } else if (kind == DUST_PROBE_SKY_PEEL) {
    /* in: {pos[3], dir[3], sin theta, cos theta, phi, sin phi, cos phi, I, Q,
     * U, V}; out: {hgfac, I, Q, U, V (rotated), r, tau, steps, pixel (-1:
     * outside the window, -2: excluded, everything but r then 0)} */
    if constexpr (CAMERA == DUST_CAMERA_POINT) {
      const double *r = in + k * 15;
      DustPhoton p;
      for (int a = 0; a < 3; ++a)
        p.pos[a] = r[a];
      dust_set_direction(p, r + 3);
      for (int j = 0; j < 5; ++j)
        p.par[j] = r[6 + j];
      for (int j = 0; j < 4; ++j)
        p.stokes[j] = r[11 + j];
      double kv[3], dist, dist2;
      if (!dust_sky_direction(cam, p.pos, kv, dist, dist2)) {
        o[5] = dist;
        o[8] = -2.;
      } else {
        unsigned long long nsteps = 0;
        o[0] = dust_scatter_towards_point(d, p, kv);
        o[6] = dust_integrate_to(g, opacity, p.pos, p.dir, p.inv_dir, dist,
                                 nsteps);
        if (!cam.pole_is_z)
          dust_sky_rotate(cam, kv, p.stokes);
        for (int j = 0; j < 4; ++j)
          o[1 + j] = p.stokes[j];
        o[5] = dist;
        o[7] = (double)nsteps;
        o[8] = (double)dust_sky_pixel(cam, kv);
      }
    }
  }
}

#endif
