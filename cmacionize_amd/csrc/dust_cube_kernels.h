/*
 * dust_cube_kernels.h - scattered-light line cubes: the Monte Carlo images of
 * dust_kernels.h resolved in radial velocity (include/cmi_gpu.h,
 * "scattered-light line cubes", has the contract; DESIGN.md 4.14 the
 * derivation). The walk is dust_packet's, random number for random number:
 * grey dust makes it independent of frequency. What is new is the Doppler
 * bookkeeping of a packet (two scalars, q and s2) and the deposit of an
 * event's addend over the velocity channels its Gaussian overlaps.
 *
 * dot3(a, b) = (a_x b_x + a_y b_y) + a_z b_z, in this order, no contraction.
 *
 * Device cube: [view][I, Q, U][pixel][channel], the channel fastest, so that
 * the spectrum of a pixel's Stokes component is contiguous (64 channels are
 * four 128-byte lines); dust_cube_reorder_kernel turns it into the ABI's
 * [channel][pixel] at download.
 *
 * The deposit (dust_cube_add) is wave-cooperative: the lanes that reach it
 * together take their events one after the other; the event's values are
 * broadcast from its lane, and the lane of rank i among the nactive active
 * ones owns the channels c_lo + i, c_lo + i + nactive, .. of the event's
 * window [c_lo, c_hi], evaluates E at their edges and issues its atomics next
 * to its neighbours'. It uses no barrier and no LDS and works for any
 * non-empty set of active lanes. An addend is w * f_c from the broadcast
 * values only: it does not depend on the lane that formed it. With
 * -DCMI_DUST_CUBE_LANE_PER_EVENT every lane deposits its own event channel by
 * channel (the same addends, the same layout), for the comparison of
 * DESIGN.md 4.14.
 */
#ifndef CMI_DUST_CUBE_KERNELS_H
#define CMI_DUST_CUBE_KERNELS_H

#include "dust_kernels.h"
#include "line_cube_kernels.h"

__device__ __forceinline__ double dust_dot3(const double a[3],
                                            const double b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

/* dot3(v_cell, k); 0 for cells at rest */
__device__ __forceinline__ double dust_cube_doppler(const DustCubeDev &cube,
                                                    int64_t cell,
                                                    const double k[3]) {
  if (!cube.velocity)
    return 0.;
  const int64_t ncell = cube.ncell;
  return (cube.velocity[cell] * k[0] + cube.velocity[ncell + cell] * k[1]) +
         cube.velocity[2 * ncell + cell] * k[2];
}

/* the cell of a scattering: floor((pos - anchor) * inv_cellside) per axis,
 * clamped into the grid (a NaN goes to 0) */
__device__ __forceinline__ int64_t dust_cube_cell(const GridDev &g,
                                                  const double pos[3]) {
  int64_t index[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double c = floor((pos[a] - g.anchor[a]) * g.inv_cellside[a]);
    index[a] = (int64_t)fmin(fmax(c, 0.), (double)(g.ncell[a] - 1));
  }
  return (index[0] * g.ncell[1] + index[1]) * g.ncell[2] + index[2];
}

/* the channels that are not wholly beyond u +- 6 b, widened by one on either
 * side against the rounding of the division (a channel of the window whose
 * f_c is 0 adds nothing all the same); empty: lo > hi */
__device__ __forceinline__ void dust_cube_window(const DustCubeDev &cube,
                                                 double u, double b, int &lo,
                                                 int &hi) {
  const double x_lo = ((u - 6. * b) - cube.vmin) / cube.dv - 1.;
  const double x_hi = ((u + 6. * b) - cube.vmin) / cube.dv + 1.;
  const double last = (double)(cube.nchan - 1);
  /* (comparisons that a NaN fails leave the whole axis) */
  lo = (x_lo > 0.) ? ((x_lo <= last) ? (int)x_lo : cube.nchan) : 0;
  hi = (x_hi < last) ? ((x_hi >= 0.) ? (int)x_hi : -1) : cube.nchan - 1;
}

/* the atomics of channel ch of one event into the spectra at `spectrum` (I),
 * + stride (Q), + 2 stride (U); returns their number */
__device__ __forceinline__ unsigned int
dust_cube_add_channel(double *spectrum, int64_t stride, int ch, double f,
                      double wi, double wq, double wu) {
  unsigned int n = 0;
  if (f != 0.) {
    if (wi != 0.) {
      atomicAdd(spectrum + ch, wi * f);
      ++n;
    }
    if (wq != 0.) {
      atomicAdd(spectrum + stride + ch, wq * f);
      ++n;
    }
    if (wu != 0.) {
      atomicAdd(spectrum + 2 * stride + ch, wu * f);
      ++n;
    }
  }
  return n;
}

/* an event's (wi, wq, wu) times f_c into channel c of the pixel's spectra,
 * for every c with f_c != 0; every lane that calls it has an event.
 * __noinline__ like its siblings: one copy of erf's
 * polynomials serves the direct light and the peel-offs of every camera. */
__device__ __noinline__ void dust_cube_add(const DustCubeDev &cube,
                                           double *spectrum, double u,
                                           double b, double wi, double wq,
                                           double wu,
                                           unsigned long long &natomics) {
  const int64_t stride = cube.npixel * cube.nchan;
  /* counted in a register, added once: natomics is a reference into the
   * caller's frame */
  unsigned long long count = 0;
#ifdef CMI_DUST_CUBE_LANE_PER_EVENT
  int lo, hi;
  dust_cube_window(cube, u, b, lo, hi);
  for (int ch = lo; ch <= hi; ++ch) {
    const double e0 = cube.vmin + (double)ch * cube.dv;
    const double e1 = cube.vmin + (double)(ch + 1) * cube.dv;
    const double f = 0.5 * (cube_E((e1 - u) / b) - cube_E((e0 - u) / b));
    count += dust_cube_add_channel(spectrum, stride, ch, f, wi, wq, wu);
  }
#else
  const unsigned long long active = __ballot(1);
  const int nactive = __popcll(active);
  const int lane = (int)(threadIdx.x & 63u);
  const int rank = __popcll(active & ((1ull << lane) - 1ull));
  for (unsigned long long m = active; m; m &= m - 1ull) {
    const int src = __ffsll((long long)m) - 1;
    double *const es = reinterpret_cast<double *>(
        __shfl(reinterpret_cast<unsigned long long>(spectrum), src, 64));
    const double eu = __shfl(u, src, 64);
    const double eb = __shfl(b, src, 64);
    const double ewi = __shfl(wi, src, 64);
    const double ewq = __shfl(wq, src, 64);
    const double ewu = __shfl(wu, src, 64);
    int lo, hi;
    dust_cube_window(cube, eu, eb, lo, hi);
    for (int ch = lo + rank; ch <= hi; ch += nactive) {
      const double e0 = cube.vmin + (double)ch * cube.dv;
      const double e1 = cube.vmin + (double)(ch + 1) * cube.dv;
      const double f = 0.5 * (cube_E((e1 - eu) / eb) - cube_E((e0 - eu) / eb));
      count += dust_cube_add_channel(es, stride, ch, f, ewi, ewq, ewu);
    }
  }
#endif
  natomics += count;
}

/* what an event adds: the trace's row of 10 ({pos[3], I, Q, U, V, weight, u,
 * b}), or the image's atomics as dust_add / dust_sky_add issue them and then
 * the cube's. pixel < 0: nothing (the caller counts it). */
template <bool TRACE>
__device__ __forceinline__ void
dust_cube_put(const DustCubeDev &cube, double *image, int view,
              const double pos[3], int64_t pixel, const double stokes[4],
              double weight, double u, double b, DustEvents &ev,
              unsigned long long &natomics) {
  if (TRACE) {
    dust_trace_row(ev, pos, stokes, weight, u, b);
    return;
  }
  if (pixel < 0)
    return;
  const double wi = weight * stokes[0], wq = weight * stokes[1],
               wu = weight * stokes[2];
  if (wi != 0.) {
    atomicAdd(image + pixel, wi);
    ++natomics;
  }
  if (wq != 0.) {
    atomicAdd(image + cube.npixel + pixel, wq);
    ++natomics;
  }
  if (wu != 0.) {
    atomicAdd(image + 2 * cube.npixel + pixel, wu);
    ++natomics;
  }
  dust_cube_add(cube,
                cube.cube + ((int64_t)view * 3 * cube.npixel + pixel) *
                                cube.nchan,
                u, b, wi, wq, wu, natomics);
}

/* one event of the parallel camera dv (view `view` of the stack) in cube
 * mode: the direct light of a packet emitted in `cell` (scattered false) or
 * the peel-off at a scattering in `cell` of a packet that came along p.dir
 * with the Doppler velocity q and the variance s2. The weights are
 * dust_packet's expressions. */
template <bool TRACE>
__device__ __noinline__ void
dust_cube_event_parallel(const GridDev &g, const DustDev &dv,
                         const DustCubeDev &cube, int view,
                         const double2 *__restrict__ opacity,
                         const DustPhoton &p, bool scattered, double weight,
                         double albedo, double q, double s2, int64_t cell,
                         DustCountersDev &c, DustEvents &ev) {
  DustPhoton peel = p;
  const double vd = dust_cube_doppler(cube, cell, dv.obs_dir);
  double w, u, b;
  if (scattered) {
    const double vk = dust_cube_doppler(cube, cell, p.dir);
    const double kd = dust_dot3(p.dir, dv.obs_dir);
    const double hgfac = dust_scatter_towards(dv, peel);
    const double tau_new = dust_integrate(g, opacity, peel.pos, peel.dir,
                                          peel.inv_dir, c.nsteps);
    w = weight * hgfac * albedo * exp(-tau_new);
    u = -(q + (vd - vk));
    b = sqrt(2. * (s2 + cube.two_sigma2 * fmax(0., 1. - kd)));
  } else {
    const double tau_old = dust_integrate(g, opacity, p.pos, dv.obs_dir,
                                          dv.obs_inv_dir, c.nsteps);
    w = 0.25 * exp(-tau_old) / M_PI;
    u = -vd;
    b = sqrt(2. * s2);
  }
  const int64_t pixel = TRACE ? -1 : dust_pixel(dv, peel.pos);
  dust_cube_put<TRACE>(cube, dv.image, view, peel.pos, pixel, peel.stokes, w,
                       u, b, ev, c.natomics);
}

/* the same for the point camera cam: dust_sky_event with u and b */
template <bool TRACE>
__device__ __noinline__ void
dust_cube_event_point(const GridDev &g, const DustDev &d,
                      const SkyCameraDev &cam, const DustCubeDev &cube,
                      int view, const double2 *__restrict__ opacity,
                      const DustPhoton &p, bool scattered, double weight,
                      double albedo, double q, double s2, int64_t cell,
                      DustCountersDev &c, DustEvents &ev) {
  DustPhoton peel = p;
  double k[3], r, r2;
  if (!dust_sky_direction(cam, peel.pos, k, r, r2)) {
    c.nexcluded += 1;
    const double nothing[4] = {0., 0., 0., 0.};
    if (TRACE)
      dust_cube_put<TRACE>(cube, cam.image, view, peel.pos, -1, nothing, 0.,
                           0., 0., ev, c.natomics);
    return;
  }
  const double vd = dust_cube_doppler(cube, cell, k);
  const double od = dust_dot3(cube.obs_velocity + 3 * view, k);
  double w, u, b;
  if (scattered) {
    const double vk = dust_cube_doppler(cube, cell, p.dir);
    const double kd = dust_dot3(p.dir, k);
    const double hgfac = dust_scatter_towards_point(d, peel, k);
    const double tau = dust_integrate_to(g, opacity, peel.pos, peel.dir,
                                         peel.inv_dir, r, c.nsteps);
    if (!cam.pole_is_z)
      dust_sky_rotate(cam, k, peel.stokes);
    w = weight * hgfac * albedo * exp(-tau);
    u = -((q + (vd - vk)) - od);
    b = sqrt(2. * (s2 + cube.two_sigma2 * fmax(0., 1. - kd)));
  } else {
    const double inv_k[3] = {1. / k[0], 1. / k[1], 1. / k[2]};
    const double tau =
        dust_integrate_to(g, opacity, peel.pos, k, inv_k, r, c.nsteps);
    w = 0.25 * exp(-tau) / M_PI;
    u = -(vd - od);
    b = sqrt(2. * s2);
  }
  const double addend = w / r2;
  const int64_t pixel = TRACE ? -1 : dust_sky_pixel(cam, k);
  if (!TRACE && pixel < 0)
    c.noutside += 1;
  dust_cube_put<TRACE>(cube, cam.image, view, peel.pos, pixel, peel.stokes,
                       addend, u, b, ev, c.natomics);
}

/* an event of dust_packet for every view of the camera, in the order and
 * with the per-view counters of dust_packet's own branches */
template <bool TRACE, int CAMERA>
__device__ __forceinline__ void
dust_cube_events(const GridDev &g, const DustDev &d,
                 const DustCamera<CAMERA> &cam, const DustCubeDev &cube,
                 const double2 *__restrict__ opacity, const DustPhoton &p,
                 bool scattered, double weight, double albedo, double q,
                 double s2, int64_t cell, DustDev &dv, SkyCameraDev &cv,
                 DustCountersDev &c, DustEvents &ev) {
  if constexpr (CAMERA == DUST_CAMERA_POINT_VIEWS) {
    if (scattered || cam.shared.direct_light) {
      for (int v = 0; v < cam.nviews; ++v) {
        dust_select_view(cam, v, cv);
        const DustCountersDev before = c;
        dust_cube_event_point<TRACE>(g, d, cv, cube, v, opacity, p, scattered,
                                     weight, albedo, q, s2, cell, c, ev);
        dust_view_count(cam.counters, v, before, c);
      }
    }
  } else if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS) {
    for (int v = 0; v < cam.nviews; ++v) {
      dust_select_view(cam, v, dv);
      const DustCountersDev before = c;
      dust_cube_event_parallel<TRACE>(g, dv, cube, v, opacity, p, scattered,
                                      weight, albedo, q, s2, cell, c, ev);
      dust_view_count(cam.counters, v, before, c);
    }
  } else if constexpr (CAMERA == DUST_CAMERA_POINT) {
    if (scattered || cam.direct_light)
      dust_cube_event_point<TRACE>(g, d, cam, cube, 0, opacity, p, scattered,
                                   weight, albedo, q, s2, cell, c, ev);
  } else {
    dust_cube_event_parallel<TRACE>(g, d, cube, 0, opacity, p, scattered,
                                    weight, albedo, q, s2, cell, c, ev);
  }
}

/* s2 of a line source: k_B T / (A m_u) + sigma_t sigma_t per cell */
__global__ void __launch_bounds__(256)
    dust_cube_line_variance_kernel(const double *__restrict__ temperature,
                                   double weight, double sigma_turb,
                                   int64_t ncell, double *__restrict__ s2) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncell)
    s2[c] = CMI_BOLTZMANN * temperature[c] / (weight * CMI_ATOMIC_MASS_UNIT) +
            sigma_turb * sigma_turb;
}

/* s2 of a field source: 0.5 b b per cell from the caller's widths; the number
 * of widths that are negative or not finite is added to *ninvalid (in the
 * style of cell_velocity_check_kernel) */
__global__ void __launch_bounds__(256)
    dust_cube_field_variance_kernel(const double *__restrict__ widths,
                                    int64_t ncell, double *__restrict__ s2,
                                    unsigned int *ninvalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell;
       c += stride) {
    const double b = widths[c];
    bad += (b >= 0. && b < HUGE_VAL) ? 0u : 1u;
    s2[c] = 0.5 * b * b;
  }
  for (int off = 32; off > 0; off >>= 1)
    bad += __shfl_down(bad, off, 64);
  if (threadIdx.x % 64 == 0 && bad)
    atomicAdd(ninvalid, bad);
}

/* one Stokes component of one view, [npixel][nchan] -> [nchan][npixel] */
__global__ void __launch_bounds__(256)
    dust_cube_reorder_kernel(const double *__restrict__ in, int64_t npixel,
                             int32_t nchan, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npixel * nchan)
    return;
  const int64_t pixel = i / nchan;
  const int32_t ch = (int32_t)(i - pixel * nchan);
  out[(int64_t)ch * npixel + pixel] = in[i];
}

#endif
