/*
 * device_dust.h - device functions of the dusty radiative transfer mode
 * (DustSimulation, src/DustSimulation.cpp:67-186): Henyey-Greenstein
 * scattering with Stokes parameters, the peel-off towards the observer, the
 * spiral galaxy source and the CCD projection.
 *
 * Random numbers of packet i (stream seed = DustSimulation:random seed,
 * iteration 0, packet i), in the order DustPhotonShootJob::execute
 * (src/DustPhotonShootJob.hpp:107-164) draws them:
 *   1   PhotonSource::get_random_photon's selector (src/PhotonSource.cpp:217;
 *       always continuous here, the value is not used)
 *   2.. SpiralGalaxyContinuousPhotonSource::get_random_incoming_direction
 *       (src/SpiralGalaxyContinuousPhotonSource.hpp:277-340), per attempt of
 *       the rejection loop: bulge/disc selector, then bulge {u, phi, cos} or
 *       disc {u1, phi, u2}; attempts repeat until the position is in the box
 *   +2  the source's isotropic direction (PhotonSource::get_random_direction),
 *       which the job throws away
 *   +2  the job's own direction {cos theta, phi}
 *   +1  the forced first optical depth, -log(1 - u (1 - exp(-tau_max)))
 *   then per scattering: DustScattering::scatter's HG cosine, its azimuth
 *   (only if |cos| != 1), and the next optical depth -log(u).
 * The CPU restatement (tests/support/dust_reference.c) draws in the same
 * order.
 *
 * The cell-luminosity source (DUST_SOURCE_CELLS, dust_emit_cells; the
 * scattered-light line images of DESIGN.md 4.8, no counterpart in the
 * reference) draws, for packet i of the same stream:
 *   1   the cell selector
 *   3   x, y, z inside the cell: lower wall + u cell side per axis
 *   2   the direction {cos theta, phi}, as the job's own above
 *   +1  the forced first optical depth, and from there on exactly the list
 *       above
 * (tests/support/scattered_line_reference.c draws in the same order.)
 *
 * Its tables, over blocks of CMI_CELL_SOURCE_BLOCK consecutive cells: C[c],
 * the running sum of the weights w >= 0 within c's block (from 0 in every
 * block, cell by cell), and B[b], the running sum of the block totals. One
 * uniform u gives t = u B[last]; b is the first block with B[b] > t (if
 * rounding put t at B[last], the first block with B[b] == B[last]); r = t -
 * B[b - 1] (B[-1] = 0); the cell is the first k of block b with C[k] > r,
 * or, if rounding leaves none, the first k with C[k] == C[last of b].
 * A cell with w == 0 is never chosen: adding 0 leaves a running sum as it
 * is, so C[k] == C[k - 1] for such a cell (C[k] == 0 for a block's first)
 * and B[b] == B[b - 1] for a block of them. The chosen block has B[b] >
 * B[b - 1] - either B[b] > t >= B[b - 1], or B[b] == B[last] > 0 is the
 * first to reach that value - so it emits and C[last of b] > 0. In it r >= 0
 * (B is monotone: t >= B[b - 1]), and the chosen k has either C[k] > r >=
 * C[k - 1] (k is the first above r), or C[k] > r >= 0 at k = first of b, or
 * is the first to reach C[last of b] > 0: in every case C[k] differs from
 * the sum before it, which w_k == 0 cannot do.
 *
 * The point camera (DUST_CAMERA_POINT, an observer inside or near the grid,
 * DESIGN.md 4.10, no counterpart in the reference) draws no random number:
 * both lists above stay true with it, and a packet's emission, optical depths
 * and scatterings are bit for bit the parallel camera's for the same seed and
 * id. Per event (the direct light at the emission point, then each peel-off
 * at a scattering point p), with the observer at o, in exactly these
 * operations (tests/support/scattered_sky_reference.c restates them):
 *   v = o - p per axis; r2 = (v_x v_x + v_y v_y) + v_z v_z; r = sqrt(r2);
 *   k = v / r per axis (a division, not a multiplication by 1 / r);
 *   1 / k per axis for the march. r2 < r_min^2: the event adds nothing and is
 *   counted (nexcluded).
 *   Scattering angles of the observer's direction (dust_scatter_towards_
 *   point): cos theta = k_z, sin theta = sqrt(fmax(1 - k_z k_z, 0)), phi =
 *   atan2(k_y, k_x) (0 where sin theta == 0), sin phi, cos phi.
 *   tau = dust_integrate_to(p, k, r): dust_integrate's march with the length
 *   s summed step by step; the step with s + ds >= r adds (r - s) kappa and
 *   ends it. An observer outside the box: the march leaves the grid first.
 *   Q, U are rotated from the meridian through the grid's z axis to the one
 *   through the frame's pole e_3 (dust_sky_rotate) unless e_3 is exactly
 *   (0, 0, 1).
 *   Pixel (dust_sky_pixel): n = -k; l = atan2(n . e_2, n . e_1), b =
 *   asin(fmin(1, fmax(-1, n . e_3))); x = l - lon_min; x -= 2 pi floor(x /
 *   (2 pi)); x += 2 pi if x < 0; x -= 2 pi if x >= 2 pi; y = b - lat_min;
 *   inside if x < lon_width and 0 <= y <= lat_width; i = (int)(nlon x /
 *   lon_width), j = (int)(nlat y / lat_width), each clamped to its last
 *   index (rounding just below the far edge, and b == lat_max itself);
 *   pixel i nlat + j. Events outside the window are counted (noutside).
 *   Addend: W / r2 times I, Q, U, with W the parallel camera's weight.
 */
#ifndef CMI_DEVICE_DUST_H
#define CMI_DEVICE_DUST_H

#include "device_transport.h"

/* scatterings after which a packet is stopped and counted (the reference has
 * no cap: the albedo is a weight, a packet scatters until it leaves) */
#define CMI_DUST_MAX_SCATTER 100000
/* attempts of the source's rejection loop after which a packet is dropped
 * and counted (the loop ends at once for a box centred on the origin; the
 * host refuses boxes that do not contain it, this bounds the rest) */
#define CMI_DUST_MAX_ATTEMPTS 1000000u

/* cells per block of the cell source's tables: the top level stays resident
 * in L2 (65 536 entries, 512 KB, at 256^3 cells) and the search within a
 * block touches 2 KB */
#define CMI_CELL_SOURCE_BLOCK 256

/* where a packet starts: template parameter of dust_packet and its kernels */
enum { DUST_SOURCE_GALAXY = 0, DUST_SOURCE_CELLS = 1 };

/* what a source reads beyond DustDev, a kernel argument of its own: nothing
 * for the spiral galaxy (its parameters are DustDev's), the tables for the
 * cells */
template <int SOURCE> struct DustSource {};
template <> struct DustSource<DUST_SOURCE_CELLS> {
  const double *block_sums; /* B[nblock] */
  const double *cell_sums;  /* C[ncell] */
  int64_t ncell, nblock;
};
typedef DustSource<DUST_SOURCE_CELLS> CellSourceDev;

/* where the peel-off goes: template parameter of dust_packet and its kernels.
 * PARALLEL: the CCD image of an observer infinitely far away (DustDev's);
 * POINT: the sky map around an observer at a point */
enum {
  DUST_CAMERA_PARALLEL = 0,
  DUST_CAMERA_POINT = 1,
  /* several cameras of one kind that share a packet's walk:
   * descriptors in device memory, one image stack [view][3][pixels] */
  DUST_CAMERA_PARALLEL_VIEWS = 2,
  DUST_CAMERA_POINT_VIEWS = 3
};

/* what a camera reads beyond DustDev, a kernel argument of its own: nothing
 * for the parallel camera */
template <int CAMERA> struct DustCamera {};
template <> struct DustCamera<DUST_CAMERA_POINT> {
  double o[3];               /* the observer */
  double e1[3], e2[3], e3[3]; /* the frame: l = 0, l = 90 deg, the pole */
  double lon_min, lat_min, lon_width, lat_width;
  int32_t nlon, nlat;
  double r_min2;        /* exclusion radius squared */
  int32_t pole_is_z;    /* e3 is exactly (0, 0, 1): Q, U are not rotated */
  int32_t direct_light; /* 0: the direct event and its march are skipped */
  double *image;        /* [3][nlon * nlat]: I, Q, U */
};
typedef DustCamera<DUST_CAMERA_POINT> SkyCameraDev;

/* one parallel view of DUST_CAMERA_PARALLEL_VIEWS: what cmi_gpu_set_ccd_image
 * puts into DustDev for it (the resolution is shared, DustDev's) */
struct DustViewDev {
  double view[5];
  double obs_dir[3];
  double obs_inv_dir[3];
  double img_anchor[2], img_sides[2];
};

/* one observer of DUST_CAMERA_POINT_VIEWS: what differs between the cameras
 * (window, resolution and direct_light are shared) */
struct SkyObserverDev {
  double o[3];
  double e1[3], e2[3], e3[3];
  double r_min2;
  int32_t pole_is_z;
};

/* per-view counters: DDA steps of the view's own marches, atomics into its
 * image, events inside the exclusion radius, events outside the window. On
 * the device each is spread over CMI_DUST_VIEW_SLOTS words, one per lane of a
 * wave ([view][counter][slot]), so that a wave's addition is one atomic
 * instruction to 64 different addresses; the host sums the slots. */
#define CMI_DUST_VIEW_COUNTERS 4
#define CMI_DUST_VIEW_SLOTS 64

template <> struct DustCamera<DUST_CAMERA_PARALLEL_VIEWS> {
  const DustViewDev *views; /* [nviews] */
  int32_t nviews;
  double *images;               /* [nviews][3][res[0] * res[1]] */
  unsigned long long *counters; /* [nviews][4][CMI_DUST_VIEW_SLOTS] */
};
template <> struct DustCamera<DUST_CAMERA_POINT_VIEWS> {
  SkyCameraDev shared; /* window, resolution, direct_light; the rest per view */
  const SkyObserverDev *views; /* [nviews] */
  int32_t nviews;
  double *images;               /* [nviews][3][nlon * nlat] */
  unsigned long long *counters; /* [nviews][4][CMI_DUST_VIEW_SLOTS] */
};

/* everything the dust kernels read, by value */
struct DustDev {
  /* DustScattering (src/DustScattering.hpp): g, g^2, 1 - g^2, 2g, 1 - g,
   * 1 / 2g, 1 + g^2, p_l, sc = 1, pc = 0, albedo */
  double hgg, g2, omg2, thgg, omhgg, od2hgg, opg2, pl, sc, pc, albedo;
  /* CCDImage (src/CCDImage.hpp:123-200): sin theta, cos theta, phi, sin phi,
   * cos phi of the observer, its direction, resolution, anchor, sides */
  double view[5];
  double obs_dir[3];
  double obs_inv_dir[3];
  int32_t res[2];
  double img_anchor[2], img_sides[2];
  double *image; /* [3][res[0] * res[1]]: I, Q, U */
  /* SpiralGalaxyContinuousPhotonSource (:98-150): box, bulge radii, disc
   * scales, corrected B/T, the disc CDF {x[n], y[n]} */
  double box_anchor[3], box_sides[3];
  double rC, rB, rJ, r_stars, h_stars, bulge_to_total;
  double rB_over_rJ_plus_rB, rC_over_rJ_plus_rC;
  const double *cdf_x, *cdf_y;
  int32_t cdf_n;
};

/* counters of a dust launch */
struct DustCountersDev {
  unsigned long long nsteps;    /* DDA steps, both marches */
  unsigned long long nscatter;  /* scattering events */
  unsigned long long ncapped;   /* packets stopped at CMI_DUST_MAX_SCATTER */
  unsigned long long natomics;  /* fp64 atomics into the image */
  unsigned long long npackets;
  unsigned long long nsource_capped; /* packets the source gave no position
                                        (CMI_DUST_MAX_ATTEMPTS) */
  /* the point camera's: events inside the exclusion radius, events outside
   * the map's window (the parallel camera leaves both 0) */
  unsigned long long nexcluded, noutside;
};

/* Photon with what the dust path reads: position, direction, its angles
 * (src/Photon.hpp:165-228) and the Stokes vector (:229-250) */
struct DustPhoton {
  double pos[3];
  double dir[3];
  double inv_dir[3];
  double par[5]; /* sin theta, cos theta, phi, sin phi, cos phi */
  double stokes[4];
};

__device__ __forceinline__ void dust_set_direction(DustPhoton &p,
                                                   const double d[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p.dir[a] = d[a];
    p.inv_dir[a] = 1. / d[a];
  }
}

/* Utilities::locate, src/Utilities.hpp:726-742 */
__device__ __forceinline__ int dust_locate(double x, const double *xarr,
                                           int length) {
  int jl = 0, ju = length;
  while (ju - jl > 1) {
    const int jm = (ju + jl) >> 1;
    if (x > xarr[jm])
      jl = jm;
    else
      ju = jm;
  }
  if (jl == length - 1)
    --jl;
  return jl;
}

/* SpiralGalaxyContinuousPhotonSource::get_random_incoming_direction without
 * the final direction (src/SpiralGalaxyContinuousPhotonSource.hpp:277-334):
 * the rejection loop until Box::inside (src/Box.hpp:191-195). false: no
 * position in the box after CMI_DUST_MAX_ATTEMPTS attempts (the reference
 * would loop on) */
__device__ inline bool dust_source_position(const DustDev &d, PacketRng &rng,
                                            double pos[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    pos[a] = d.box_anchor[a] - d.box_sides[a];
  auto inside = [&]() {
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      in &= pos[a] >= d.box_anchor[a] &&
            pos[a] < d.box_anchor[a] + d.box_sides[a];
    return in;
  };
  for (uint32_t attempt = 0; !inside(); ++attempt) {
    if (attempt == CMI_DUST_MAX_ATTEMPTS)
      return false;
    const double x_bulge = rng.next();
    if (x_bulge <= d.bulge_to_total) {
      const double u = rng.next();
      const double A =
          u * d.rB_over_rJ_plus_rB + (1. - u) * d.rC_over_rJ_plus_rC;
      const double r = d.rJ / (1. / A - 1.);
      const double phi = 2. * M_PI * rng.next();
      const double cost = 2. * rng.next() - 1.;
      const double sint = sqrt(fmax(1. - cost * cost, 0.));
      pos[0] = r * sint * cos(phi);
      pos[1] = r * sint * sin(phi);
      pos[2] = r * cost;
    } else {
      const double u1 = 2. * rng.next() - 1.;
      const double z = (u1 > 0.) ? -d.h_stars * log(u1) : d.h_stars * log(-u1);
      const double phi = 2. * M_PI * rng.next();
      const double u2 = rng.next();
      const int i = dust_locate(u2, d.cdf_y, d.cdf_n);
      const double w = d.cdf_x[i] + (u2 - d.cdf_y[i]) /
                                        (d.cdf_y[i + 1] - d.cdf_y[i]) *
                                        (d.cdf_x[i + 1] - d.cdf_x[i]);
      pos[0] = w * cos(phi);
      pos[1] = w * sin(phi);
      pos[2] = z;
    }
  }
  return true;
}

/* the draws of DustPhotonShootJob::execute up to the first march
 * (src/DustPhotonShootJob.hpp:113-127): selector, position, the discarded
 * source direction, the job's direction; Stokes (1, 0, 0, 0)
 * (src/Photon.hpp:89-92); false if the source found no position */
__device__ __noinline__ bool dust_emit(const DustDev &d, PacketRng &rng,
                                       DustPhoton &p) {
  (void)rng.next();
  if (!dust_source_position(d, rng, p.pos))
    return false;
  (void)rng.next();
  (void)rng.next();
  const double cost = 2. * rng.next() - 1.;
  const double sint = sqrt(fmax(1. - cost * cost, 0.));
  const double phi = 2. * M_PI * rng.next();
  const double cosp = cos(phi);
  const double sinp = sin(phi);
  const double dir[3] = {sint * cosp, sint * sinp, cost};
  dust_set_direction(p, dir);
  p.par[0] = sint;
  p.par[1] = cost;
  p.par[2] = phi;
  p.par[3] = sinp;
  p.par[4] = cosp;
  p.stokes[0] = 1.;
  p.stokes[1] = 0.;
  p.stokes[2] = 0.;
  p.stokes[3] = 0.;
  return true;
}

/* first index in [lo, hi) with a[i] > x, or hi (a is non-decreasing) */
__device__ __forceinline__ int64_t cell_source_first_above(const double *a,
                                                           int64_t lo,
                                                           int64_t hi,
                                                           double x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] > x)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

/* first index in [lo, hi) with a[i] == a[hi - 1] */
__device__ __forceinline__ int64_t cell_source_first_last(const double *a,
                                                          int64_t lo,
                                                          int64_t hi) {
  const double last = a[hi - 1];
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] == last)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

/* the selection rule of the header comment for one uniform */
__device__ __forceinline__ int64_t cell_source_select(const CellSourceDev &s,
                                                      double u) {
  const double t = u * s.block_sums[s.nblock - 1];
  int64_t b = cell_source_first_above(s.block_sums, 0, s.nblock, t);
  if (b == s.nblock)
    b = cell_source_first_last(s.block_sums, 0, s.nblock);
  const double r = t - (b > 0 ? s.block_sums[b - 1] : 0.);
  const int64_t lo = b * CMI_CELL_SOURCE_BLOCK;
  const int64_t hi = (lo + CMI_CELL_SOURCE_BLOCK < s.ncell)
                         ? lo + CMI_CELL_SOURCE_BLOCK
                         : s.ncell;
  int64_t k = cell_source_first_above(s.cell_sums, lo, hi, r);
  if (k == hi)
    k = cell_source_first_last(s.cell_sums, lo, hi);
  return k;
}

/* the draws of a packet of the cell source up to the first march: the cell,
 * a position inside it, the direction as dust_emit's own; Stokes (1, 0, 0,
 * 0). The grid is whole (the host refuses blocks of a decomposed one). */
__device__ __noinline__ int64_t dust_emit_cells(const GridDev &g,
                                                const CellSourceDev &s,
                                                PacketRng &rng,
                                                DustPhoton &p) {
  const int64_t cell = cell_source_select(s, rng.next());
  const int64_t nyz = (int64_t)g.ncell[1] * g.ncell[2];
  const int64_t index[3] = {cell / nyz, (cell / g.ncell[2]) % g.ncell[1],
                            cell % g.ncell[2]};
#pragma unroll
  for (int a = 0; a < 3; ++a)
    p.pos[a] = (g.anchor[a] + g.cellside[a] * (double)index[a]) +
               rng.next() * g.cellside[a];
  const double cost = 2. * rng.next() - 1.;
  const double sint = sqrt(fmax(1. - cost * cost, 0.));
  const double phi = 2. * M_PI * rng.next();
  const double cosp = cos(phi);
  const double sinp = sin(phi);
  const double dir[3] = {sint * cosp, sint * sinp, cost};
  dust_set_direction(p, dir);
  p.par[0] = sint;
  p.par[1] = cost;
  p.par[2] = phi;
  p.par[3] = sinp;
  p.par[4] = cosp;
  p.stokes[0] = 1.;
  p.stokes[1] = 0.;
  p.stokes[2] = 0.;
  p.stokes[3] = 0.;
  return cell;
}

/* the march's packet for a photon: dust opacity records are {n kappa x_H, 0},
 * so sigma_H = 1 and sigma_He_corr = 0 give tau = ds n kappa x_H
 * (src/DensityGrid.hpp:118-140 at sigma_He = 0, x_He = 0) */
__device__ __forceinline__ void dust_march_packet(const GridDev &g,
                                                  const double pos[3],
                                                  const double dir[3],
                                                  const double inv_dir[3],
                                                  Packet<false> &q) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q.pos[a] = pos[a];
    q.dir[a] = dir[a];
    q.inv_dir[a] = inv_dir[a];
  }
  q.sigma_H = 1.;
  q.sigma_He_corr = 0.;
  locate_cell(g, q);
}

/* CartesianDensityGrid::integrate_optical_depth,
 * src/CartesianDensityGrid.cpp:328-363; `cells` (if not null) receives the
 * first max_cells cells */
__device__ __noinline__ double
dust_integrate(const GridDev &g, const double2 *__restrict__ opacity,
               const double pos[3], const double dir[3],
               const double inv_dir[3], unsigned long long &nsteps,
               double *cells = nullptr, int max_cells = 0) {
  Packet<false> q;
  dust_march_packet(g, pos, dir, inv_dir, q);
  q.tau = HUGE_VAL; /* never reached: the march ends at the box edge */
  double optical_depth = 0.;
  int n = 0;
  while (is_inside(g, q)) {
    int64_t cell;
    double2 kappa;
    const double ds = dda_step<false>(g, opacity, q, cell, kappa);
    optical_depth += ds * fmax(kappa.x, 0.);
    if (cells && n < max_cells)
      cells[n] = (double)cell;
    ++n;
  }
  nsteps += n;
  return optical_depth;
}

/* CartesianDensityGrid::interact, src/CartesianDensityGrid.cpp:375-452,
 * without the integrals: moves the photon; false = DensityGrid::end() (the
 * photon left the box, or no step was taken) */
__device__ __noinline__ bool dust_interact(const GridDev &g,
                                     const double2 *__restrict__ opacity,
                                     DustPhoton &p, double optical_depth,
                                     unsigned long long &nsteps) {
  Packet<false> q;
  dust_march_packet(g, p.pos, p.dir, p.inv_dir, q);
  q.tau = optical_depth;
  int n = 0;
  while (is_inside(g, q) && q.tau > 0.) {
    int64_t cell;
    double2 kappa;
    (void)dda_step<false>(g, opacity, q, cell, kappa);
    ++n;
  }
  nsteps += n;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    p.pos[a] = q.pos[a];
  return n > 0 && is_inside(g, q);
}

/* White (1979), eqs. 3-6: the elements P1..P4 of the dust's scattering matrix
 * for the cosine mu of the scattering angle. The skew of eq. 6 is taken in
 * radians for a scattering and in degrees for a peel-off, as the reference
 * does in the two places (src/DustScattering.cpp:138-147, :374-380); the two
 * round differently. */
struct DustPhase {
  double P1, P2, P3, P4;
};

__device__ __forceinline__ DustPhase dust_phase(const DustDev &d, double mu,
                                                bool degrees) {
  DustPhase m;
  const double mu2 = mu * mu;
  m.P1 = d.omg2 * pow(d.opg2 - d.thgg * mu, -1.5);
  const double q = 1. / (1. + mu2);
  m.P2 = -d.pl * m.P1 * (1. - mu2) * q;
  m.P3 = 2. * m.P1 * mu * q;
  double c;
  if (degrees) {
    const double t = acos(mu) * 180. * M_1_PI;
    const double f = 3.13 * t * exp(-7. * t / 180.);
    c = cos((t + d.sc * f) * M_PI / 180.);
  } else {
    const double t = acos(mu);
    c = cos(t + d.sc * 3.13 * t * exp(-7. * t * M_1_PI));
  }
  const double c2 = c * c;
  m.P4 = -d.pc * m.P1 * (1. - c2) / (1. + c2);
  return m;
}

/* Code & Whitney (1995), eq. 2: the Stokes vector rotated into the
 * scattering plane, scattered, rotated out of it. (c1, s1) and (c2, s2) are
 * cos and sin of twice the two rotation angles; for an azimuth above pi the
 * reference measures the angle the other way round, which flips the sign of
 * every term odd in s1 or s2 (src/DustScattering.cpp:177-282, :391-491).
 * `s` is normalised to I = 1 on the way in and scaled back on the way out. */
__device__ __forceinline__ void dust_apply_phase(const DustPhase &m, double c1,
                                                 double s1, double c2,
                                                 double s2, bool mirror,
                                                 double s[4]) {
  const double I0 = s[0], r = 1. / I0;
  const double v[4] = {1., s[1] * r, s[2] * r, s[3] * r};
  const double ss = s2 * s1, cc = c2 * c1, sc = s2 * c1, cs = c2 * s1;
  const double row0[3] = {m.P1, m.P2 * c1, mirror ? m.P2 * s1 : -m.P2 * s1};
  const double row1[4] = {m.P2 * c2, m.P1 * cc - m.P3 * ss,
                          mirror ? m.P1 * cs + m.P3 * sc
                                 : -m.P1 * cs - m.P3 * sc,
                          mirror ? -m.P4 * s2 : m.P4 * s2};
  const double row2[4] = {mirror ? -m.P2 * s2 : m.P2 * s2,
                          mirror ? -m.P1 * sc - m.P3 * cs
                                 : m.P1 * sc + m.P3 * cs,
                          -m.P1 * ss + m.P3 * cc, -m.P4 * c2};
  const double row3[3] = {mirror ? -m.P4 * s1 : m.P4 * s1, m.P4 * c1, m.P3};
  const double inv = 1. / m.P1;
  const double o0 = (row0[0] * v[0] + row0[1] * v[1] + row0[2] * v[2]) * inv;
  const double o1 = (row1[0] * v[0] + row1[1] * v[1] + row1[2] * v[2] +
                     row1[3] * v[3]) *
                    inv;
  const double o2 = (row2[0] * v[0] + row2[1] * v[1] + row2[2] * v[2] +
                     row2[3] * v[3]) *
                    inv;
  const double o3 = (row3[0] * v[1] + row3[1] * v[2] + row3[2] * v[3]) * inv;
  s[0] = o0 * I0;
  s[1] = o1 * I0;
  s[2] = o2 * I0;
  s[3] = o3 * I0;
}

/* cos and sin of twice an angle given its cos and sin */
__device__ __forceinline__ void dust_double_angle(double c, double s,
                                                  double &c2, double &s2) {
  c2 = 2. * c * c - 1.;
  s2 = 2. * s * c;
}

/* DustScattering::scatter, src/DustScattering.cpp:41-323: a scattering
 * angle from the HG phase function (Witt 1977, eq. 19), an azimuth of the
 * scattering plane, the new direction (Yusef-Zadeh, Morris & White 1984,
 * eq. 16) and the Stokes vector through dust_apply_phase */
__device__ __noinline__ void dust_scatter(const DustDev &d, PacketRng &rng,
                                          DustPhoton &p) {
  const double t = d.omg2 / (d.omhgg + d.thgg * rng.next());
  const double mu = fmin(1., fmax(-1., d.od2hgg * (d.opg2 - t * t)));
  if (fabs(mu) == 1.) {
    /* straight on: nothing changes; straight back: the direction and U
     * change sign, phi turns by pi */
    if (mu == -1.) {
      p.stokes[2] = -p.stokes[2];
      const double back[3] = {-p.dir[0], -p.dir[1], -p.dir[2]};
      dust_set_direction(p, back);
      p.par[1] = -p.par[1];
      p.par[2] += M_PI;
      p.par[3] = -p.par[3];
      p.par[4] = -p.par[4];
    }
    return;
  }
  const DustPhase m = dust_phase(d, mu, false);
  const double smu = sqrt(fmax(0., 1. - mu * mu));
  const double psi = 2. * M_PI * rng.next();
  const bool mirror = psi > M_PI;
  const double a1 = mirror ? 2. * M_PI - psi : psi;
  const double c1 = cos(a1), s1 = sin(a1);
  const double st0 = p.par[0], ct0 = p.par[1];
  const double ct = ct0 * mu + st0 * smu * c1;
  double st, s2, c2;
  if (fabs(ct) < 1.) {
    st = fabs(sqrt(1. - ct * ct));
    s2 = s1 * st0 / st;
    c2 = (ct0 - ct * mu) / (st * smu);
  } else {
    st = 0.;
    s2 = 0.;
    c2 = ct >= 1. ? -1. : 1.;
  }
  const double dphi = acos(fmin(1., fmax(-1., -c2 * c1 + s2 * s1 * mu)));
  double ph = mirror ? p.par[2] + dphi : p.par[2] - dphi;
  if (ph > 2. * M_PI)
    ph -= 2. * M_PI;
  if (ph < 0.)
    ph += 2. * M_PI;
  double cc1, ss1, cc2, ss2;
  dust_double_angle(c1, s1, cc1, ss1);
  dust_double_angle(c2, s2, cc2, ss2);
  dust_apply_phase(m, cc1, ss1, cc2, ss2, mirror, p.stokes);
  const double cph = cos(ph), sph = sin(ph);
  const double dir[3] = {st * cph, st * sph, ct};
  dust_set_direction(p, dir);
  p.par[0] = st;
  p.par[1] = ct;
  p.par[2] = ph;
  p.par[3] = sph;
  p.par[4] = cph;
}

/* The Stokes update of DustScattering::scatter_towards,
 * src/DustScattering.cpp:325-500, for an observer whose direction has the
 * polar angle of sine view[0] and cosine view[1] and the azimuth view[2], at
 * the cosine mu of the scattering angle: the body that
 * dust_scatter_towards and dust_scatter_towards_point share. */
__device__ __forceinline__ void dust_scatter_stokes(const DustDev &d,
                                                    const double *view,
                                                    double mu, DustPhoton &p) {
  if (fabs(mu) == 1.) {
    if (mu == -1.)
      p.stokes[2] = -p.stokes[2];
  } else {
    const DustPhase m = dust_phase(d, mu, true);
    const double smu = sqrt(-(mu * mu - 1.));
    const double st0 = p.par[0], ct0 = p.par[1];
    const double so = view[0], co = view[1];
    double r1;
    if (st0 == 0.) {
      r1 = M_PI;
    } else {
      const double y = sin(p.par[2] - view[2] - M_PI) * so / smu;
      const double x = (co - ct0 * mu) / (st0 * smu);
      r1 = atan2(y, x) + M_PI;
    }
    const bool mirror = r1 > M_PI;
    const double a1 = mirror ? 2. * M_PI - r1 : r1;
    const double c1 = cos(a1), s1 = sin(a1);
    double s2, c2;
    if (fabs(co) < 1.) {
      s2 = s1 * st0 / so;
      const double den = so * smu;
      c2 = ct0 / den - co * mu / den;
    } else {
      s2 = 0.;
      c2 = co >= 1. ? -1. : 1.;
    }
    double cc1, ss1, cc2, ss2;
    dust_double_angle(c1, s1, cc1, ss1);
    dust_double_angle(c2, s2, cc2, ss2);
    dust_apply_phase(m, cc1, ss1, cc2, ss2, mirror, p.stokes);
  }
}

/* DustScattering::scatter_towards, src/DustScattering.cpp:325-518: the
 * photon's Stokes vector after a scattering towards the observer (direction
 * d.obs_dir, angles d.view); the photon takes the observer's direction.
 * Returns the HG phase function per steradian. */
__device__ __noinline__ double dust_scatter_towards(const DustDev &d,
                                                    DustPhoton &p) {
  const double mu = d.obs_dir[0] * p.dir[0] + d.obs_dir[1] * p.dir[1] +
                    d.obs_dir[2] * p.dir[2];
  dust_scatter_stokes(d, d.view, mu, p);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p.dir[a] = d.obs_dir[a];
    p.inv_dir[a] = d.obs_inv_dir[a];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k)
    p.par[k] = d.view[k];
  return 0.25 * d.omg2 * pow(d.opg2 - d.thgg * mu, -1.5) * M_1_PI;
}

/* dust_integrate's march from pos along dir, cut at the length r (the point
 * camera's observer): the travelled length s is summed step by step, the step
 * in which s + ds >= r adds (r - s) kappa and ends the march. If the grid
 * ends first (an observer outside the box) this is dust_integrate. */
__device__ __noinline__ double
dust_integrate_to(const GridDev &g, const double2 *__restrict__ opacity,
                  const double pos[3], const double dir[3],
                  const double inv_dir[3], double r,
                  unsigned long long &nsteps) {
  Packet<false> q;
  dust_march_packet(g, pos, dir, inv_dir, q);
  q.tau = HUGE_VAL;
  double optical_depth = 0., s = 0.;
  int n = 0;
  while (is_inside(g, q)) {
    int64_t cell;
    double2 kappa;
    const double ds = dda_step<false>(g, opacity, q, cell, kappa);
    ++n;
    const double k = fmax(kappa.x, 0.);
    if (s + ds >= r) {
      optical_depth += (r - s) * k;
      break;
    }
    optical_depth += ds * k;
    s += ds;
  }
  nsteps += n;
  return optical_depth;
}

/* dust_scatter_towards for an observer in the direction k (a unit vector)
 * from the photon: the same operations with the observer's angles computed
 * from k (the header comment lists them); the photon takes k, 1 / k and
 * those angles. Returns the HG phase function per steradian. (The CPU
 * restatements have scatter_towards and scatter_towards_point.) */
__device__ __noinline__ double
dust_scatter_towards_point(const DustDev &d, DustPhoton &p,
                           const double k[3]) {
  const double co = k[2];
  const double so = sqrt(fmax(1. - co * co, 0.));
  const double pho = so == 0. ? 0. : atan2(k[1], k[0]);
  const double view[5] = {so, co, pho, sin(pho), cos(pho)};
  const double mu = k[0] * p.dir[0] + k[1] * p.dir[1] + k[2] * p.dir[2];
  dust_scatter_stokes(d, view, mu, p);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p.dir[a] = k[a];
    p.inv_dir[a] = 1. / k[a];
  }
#pragma unroll
  for (int j = 0; j < 5; ++j)
    p.par[j] = view[j];
  return 0.25 * d.omg2 * pow(d.opg2 - d.thgg * mu, -1.5) * M_1_PI;
}

/* the point camera's direction and distance from pos to the observer (the
 * header comment has the operations); false inside the exclusion radius */
__device__ __forceinline__ bool dust_sky_direction(const SkyCameraDev &cam,
                                                   const double pos[3],
                                                   double k[3], double &r,
                                                   double &r2) {
  const double v[3] = {cam.o[0] - pos[0], cam.o[1] - pos[1],
                       cam.o[2] - pos[2]};
  r2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  r = sqrt(r2);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    k[a] = v[a] / r;
  return !(r2 < cam.r_min2);
}

/* Q, U of a photon flying along k, referred by dust_scatter_towards* to the
 * meridian through k and the grid's z axis, referred to the meridian through
 * k and the frame's pole e3 instead: a rotation by twice the angle chi from
 * the projection N_z = z - (z . k) k to N_e = e3 - (e3 . k) k in the plane
 * perpendicular to k, cos chi = N_z . N_e / (|N_z| |N_e|), sin chi = (N_z x
 * N_e) . k / (|N_z| |N_e|); chi = 0 where a projection vanishes. The sign
 * (Q' = Q cos 2 chi - U sin 2 chi, U' = Q sin 2 chi + U cos 2 chi) follows
 * the handedness of the reference's U (pinned by the
 * polarisation-pattern test). */
__device__ __forceinline__ void dust_sky_rotate(const SkyCameraDev &cam,
                                                const double k[3],
                                                double stokes[4]) {
  const double zk = k[2];
  const double ek = cam.e3[0] * k[0] + cam.e3[1] * k[1] + cam.e3[2] * k[2];
  const double nz[3] = {-zk * k[0], -zk * k[1], 1. - zk * k[2]};
  const double ne[3] = {cam.e3[0] - ek * k[0], cam.e3[1] - ek * k[1],
                        cam.e3[2] - ek * k[2]};
  const double lz = sqrt(nz[0] * nz[0] + nz[1] * nz[1] + nz[2] * nz[2]);
  const double le = sqrt(ne[0] * ne[0] + ne[1] * ne[1] + ne[2] * ne[2]);
  if (lz == 0. || le == 0.)
    return;
  const double norm = lz * le;
  const double cx[3] = {nz[1] * ne[2] - nz[2] * ne[1],
                        nz[2] * ne[0] - nz[0] * ne[2],
                        nz[0] * ne[1] - nz[1] * ne[0]};
  const double cchi = (nz[0] * ne[0] + nz[1] * ne[1] + nz[2] * ne[2]) / norm;
  const double schi = (cx[0] * k[0] + cx[1] * k[1] + cx[2] * k[2]) / norm;
  double c2, s2;
  dust_double_angle(cchi, schi, c2, s2);
  const double q = stokes[1], u = stokes[2];
  stokes[1] = q * c2 - u * s2;
  stokes[2] = q * s2 + u * c2;
}

/* the pixel (i * nlat + j, DESIGN.md 4.9's order) of the sky direction -k,
 * or -1 outside the map's window (the header comment has the operations) */
__device__ __forceinline__ int64_t dust_sky_pixel(const SkyCameraDev &cam,
                                                  const double k[3]) {
  const double n[3] = {-k[0], -k[1], -k[2]};
  const double n1 = n[0] * cam.e1[0] + n[1] * cam.e1[1] + n[2] * cam.e1[2];
  const double n2 = n[0] * cam.e2[0] + n[1] * cam.e2[1] + n[2] * cam.e2[2];
  const double n3 = n[0] * cam.e3[0] + n[1] * cam.e3[1] + n[2] * cam.e3[2];
  const double l = atan2(n2, n1);
  const double b = asin(fmin(1., fmax(-1., n3)));
  double x = l - cam.lon_min;
  x -= 2. * M_PI * floor(x / (2. * M_PI));
  if (x < 0.)
    x += 2. * M_PI;
  if (x >= 2. * M_PI)
    x -= 2. * M_PI;
  const double y = b - cam.lat_min;
  if (!(x < cam.lon_width) || !(y >= 0.) || !(y <= cam.lat_width))
    return -1;
  int32_t i = (int32_t)(cam.nlon * x / cam.lon_width);
  int32_t j = (int32_t)(cam.nlat * y / cam.lat_width);
  /* n x / width can round up to n just below the far edge, and b == lat_max
   * itself belongs to the last row */
  if (i >= cam.nlon)
    i = cam.nlon - 1;
  if (j >= cam.nlat)
    j = cam.nlat - 1;
  return (int64_t)i * cam.nlat + j;
}

/* CCDImage::add_photon, src/CCDImage.hpp:242-270: the pixel (ix * ny + iy)
 * a position projects to, or -1 outside the image */
__device__ __forceinline__ int64_t dust_pixel(const DustDev &d,
                                              const double pos[3]) {
  const double cospo = d.view[4], sinpo = d.view[3], costo = d.view[1],
               sinto = d.view[0];
  double xphoton = pos[1] * cospo - pos[0] * sinpo;
  double yphoton =
      pos[2] * sinto - pos[1] * costo * sinpo - pos[0] * costo * cospo;
  if (xphoton >= d.img_anchor[0] && yphoton >= d.img_anchor[1]) {
    xphoton -= d.img_anchor[0];
    yphoton -= d.img_anchor[1];
    if (xphoton < d.img_sides[0] && yphoton < d.img_sides[1]) {
      const uint32_t ix = (uint32_t)(d.res[0] * xphoton / d.img_sides[0]);
      const uint32_t iy = (uint32_t)(d.res[1] * yphoton / d.img_sides[1]);
      /* res x / sides can round up to res just below the far edge; the
       * reference would index past its vectors there */
      if (ix < (uint32_t)d.res[0] && iy < (uint32_t)d.res[1])
        return (int64_t)ix * d.res[1] + iy;
    }
  }
  return -1;
}

#endif
