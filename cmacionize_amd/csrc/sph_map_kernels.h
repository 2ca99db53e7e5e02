/*
 * sph_map_kernels.h - the two SPH mappings on the device (cmi_gpu.h, "SPH
 * mappings"): sums of a compact kernel W over (particle, cell midpoint) pairs,
 *
 *   cells <- particles   out[k][c] = sum_i a_k[i] W(|c - p_i|, h_i)
 *   particles <- cells   out[i]    = sum_c W(|c - p_i|, h_i) g[c]
 *
 * both as gathers: every output has one owner that sums in registers and
 * writes once, so there is no floating-point atomic anywhere.
 *
 * cells <- particles: the grid is cut into tiles of 4 x 8 x 8 cells
 * (sph_map_plan.h), one workgroup of 256 lanes per tile, one lane per cell.
 * sph_tile_count_kernel counts, per tile, the particles whose reach box
 * touches it (integer atomics), the host scans the counts, and
 * sph_tile_fill_kernel writes the particle indices behind each tile's
 * offset. sph_cells_kernel stages a tile's list through LDS in chunks of
 * CMI_SPH_STAGE_CHUNK records {x, y, z, h, 1/h^3, a_0..a_K-1}; all lanes read
 * the same record at the same time (an LDS broadcast) and test r^2 against
 * the reach before they pay for the square root.
 *
 * particles <- cells: the host splits the particles by the number of
 * candidate midpoints in their reach box. sph_particles_lane_kernel gives a
 * particle of up to CMI_SPH_LANE_CANDIDATES candidates one lane;
 * sph_particles_wave_kernel gives a larger one a wave, whose lanes stride the
 * candidates and add their partial sums up in a fixed tree.
 *
 * fp64 throughout. With -ffp-contract=off the midpoints are the host grid's
 * to the bit.
 */
#ifndef CMI_SPH_MAP_KERNELS_H
#define CMI_SPH_MAP_KERNELS_H

#include "sph_map_plan.h"

#include <hip/hip_runtime.h>

/* W(r, h) times h^3 for a pair with r^2 below the reach squared */
template <int FORM>
static __device__ __forceinline__ double cmi_sph_shape(double r, double h) {
  if (FORM == CMI_SPH_FORM_SPLINE_H) {
    /* cubic_spline_kernel, src/CubicSplineKernel.hpp:36-59 */
    const double KC1 = 2.546479089470;
    const double KC2 = 15.278874536822;
    const double KC5 = 5.092958178941;
    const double u = r / h;
    if (u < 1.) {
      if (u < 0.5)
        return KC1 + KC2 * (u - 1.) * u * u;
      return KC5 * (1. - u) * (1. - u) * (1. - u);
    }
    return 0.;
  } else {
    /* PhantomSnapshotDensityFunction::kernel, :48-64 */
    const double INV_PI = 0.318309886183790671538;
    const double q = r / h;
    if (q < 1.) {
      const double q2 = q * q;
      return (1. - 1.5 * q2 + 0.75 * q2 * q) * INV_PI;
    }
    if (q < 2.) {
      const double c = 2. - q, c2 = c * c;
      return 0.25 * c2 * c * INV_PI;
    }
    return 0.;
  }
}

/* --------------------------------------------------- the tile lists -- */

template <int FORM>
__global__ void __launch_bounds__(256)
sph_tile_count_kernel(SphMapGeometry g, int64_t n,
                      const double *__restrict__ positions,
                      const double *__restrict__ h,
                      unsigned int *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const double p[3] = {positions[3 * i], positions[3 * i + 1],
                       positions[3 * i + 2]};
  SphTileRange r;
  if (cmi_sph_particle_tiles(g, p, cmi_sph_reach(FORM, h[i]), r) == 0)
    return;
  for (int kx = 0; kx < r.n[0]; ++kx)
    for (int tx = r.lo[0][kx]; tx <= r.hi[0][kx]; ++tx)
      for (int ky = 0; ky < r.n[1]; ++ky)
        for (int ty = r.lo[1][ky]; ty <= r.hi[1][ky]; ++ty)
          for (int kz = 0; kz < r.n[2]; ++kz)
            for (int tz = r.lo[2][kz]; tz <= r.hi[2][kz]; ++tz)
              atomicAdd(&counts[((size_t)tx * g.ntile[1] + ty) * g.ntile[2] +
                                tz],
                        1u);
}

/* cursors: a copy of the tiles' offsets, advanced here */
template <int FORM>
__global__ void __launch_bounds__(256)
sph_tile_fill_kernel(SphMapGeometry g, int64_t n,
                     const double *__restrict__ positions,
                     const double *__restrict__ h,
                     unsigned int *__restrict__ cursors,
                     const unsigned int *__restrict__ ends,
                     uint32_t *__restrict__ list) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const double p[3] = {positions[3 * i], positions[3 * i + 1],
                       positions[3 * i + 2]};
  SphTileRange r;
  if (cmi_sph_particle_tiles(g, p, cmi_sph_reach(FORM, h[i]), r) == 0)
    return;
  for (int kx = 0; kx < r.n[0]; ++kx)
    for (int tx = r.lo[0][kx]; tx <= r.hi[0][kx]; ++tx)
      for (int ky = 0; ky < r.n[1]; ++ky)
        for (int ty = r.lo[1][ky]; ty <= r.hi[1][ky]; ++ty)
          for (int kz = 0; kz < r.n[2]; ++kz)
            for (int tz = r.lo[2][kz]; tz <= r.hi[2][kz]; ++tz) {
              const size_t tile =
                  ((size_t)tx * g.ntile[1] + ty) * g.ntile[2] + tz;
              const unsigned int at = atomicAdd(&cursors[tile], 1u);
              /* (the count and the fill run the same arithmetic on the same
               * numbers; the bound keeps a disagreement inside the list) */
              if (at < ends[tile])
                list[at] = (uint32_t)i;
            }
}

/* --------------------------------------------------- cells <- particles -- */

/* offsets[tile] .. offsets[tile + 1]: the tile's part of the list */
template <int FORM, int K, bool PERIODIC>
__global__ void __launch_bounds__(CMI_SPH_TILE_CELLS)
sph_cells_kernel(SphMapGeometry g, int64_t n,
                 const double *__restrict__ positions,
                 const double *__restrict__ h,
                 const double *__restrict__ amplitudes, /* [K][n] */
                 const unsigned int *__restrict__ offsets,
                 const uint32_t *__restrict__ list,
                 double *__restrict__ out /* [K][ncells] */) {
  constexpr int REC = 5 + K;
  __shared__ double stage[CMI_SPH_STAGE_CHUNK * REC];

  const int tile = blockIdx.x;
  const int tz = tile % g.ntile[2];
  const int ty = (tile / g.ntile[2]) % g.ntile[1];
  const int tx = tile / (g.ntile[2] * g.ntile[1]);
  const int lane = threadIdx.x;
  const int ix = tx * CMI_SPH_TILE_X + (lane >> 6);
  const int iy = ty * CMI_SPH_TILE_Y + ((lane >> 3) & 7);
  const int iz = tz * CMI_SPH_TILE_Z + (lane & 7);
  const bool inside = ix < g.ncell[0] && iy < g.ncell[1] && iz < g.ncell[2];
  const double c[3] = {cmi_sph_midpoint(g, 0, ix), cmi_sph_midpoint(g, 1, iy),
                       cmi_sph_midpoint(g, 2, iz)};
  double sum[K];
#pragma unroll
  for (int k = 0; k < K; ++k)
    sum[k] = 0.;

  const unsigned int begin = offsets[tile], end = offsets[tile + 1];
  for (unsigned int base = begin; base < end; base += CMI_SPH_STAGE_CHUNK) {
    const int count = (int)min((unsigned int)CMI_SPH_STAGE_CHUNK, end - base);
    __syncthreads(); /* the last chunk has been read */
    if (lane < count) {
      const size_t i = list[base + lane];
      double *rec = stage + lane * REC;
      const double hi = h[i];
      rec[0] = positions[3 * i];
      rec[1] = positions[3 * i + 1];
      rec[2] = positions[3 * i + 2];
      rec[3] = hi;
      rec[4] = 1. / (hi * hi * hi);
#pragma unroll
      for (int k = 0; k < K; ++k)
        rec[5 + k] = amplitudes[(size_t)k * n + i];
    }
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const double *rec = stage + j * REC;
      double d[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        d[a] = c[a] - rec[a];
        if (PERIODIC) {
          if (2. * d[a] < -g.box[a])
            d[a] += g.box[a];
          if (2. * d[a] >= g.box[a])
            d[a] -= g.box[a];
        }
      }
      const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      const double hj = rec[3];
      const double reach = cmi_sph_reach(FORM, hj);
      if (r2 < reach * reach) {
        const double w = cmi_sph_shape<FORM>(sqrt(r2), hj) * rec[4];
#pragma unroll
        for (int k = 0; k < K; ++k)
          sum[k] += rec[5 + k] * w;
      }
    }
  }
  if (inside) {
    const size_t ncells = (size_t)g.ncell[0] * g.ncell[1] * g.ncell[2];
    const size_t cell = ((size_t)ix * g.ncell[1] + iy) * g.ncell[2] + iz;
#pragma unroll
    for (int k = 0; k < K; ++k)
      out[(size_t)k * ncells + cell] = sum[k];
  }
}

/* --------------------------------------------------- particles <- cells -- */

/* the candidate midpoints of one particle, flattened z-fastest */
struct SphCandidates {
  int32_t n[3], lo[3][3], hi[3][3];
  int32_t count[3];
};
static __device__ __forceinline__ int32_t
cmi_sph_candidates(const SphMapGeometry &g, const double p[3], double reach,
                   SphCandidates &c) {
  int32_t total = 1; /* (the host declines what does not fit) */
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c.n[a] = cmi_sph_axis_cells(g, a, p[a], reach, c.lo[a], c.hi[a]);
    c.count[a] = (int32_t)cmi_sph_interval_cells(c.n[a], c.lo[a], c.hi[a]);
    total *= c.count[a];
  }
  return total;
}
/* the cell index along axis a of the candidate's ordinal there */
static __device__ __forceinline__ int32_t
cmi_sph_candidate_cell(const SphCandidates &c, int a, int32_t ordinal) {
  int32_t cell = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < c.n[a]) {
      const int32_t len = c.hi[a][k] - c.lo[a][k] + 1;
      if (ordinal >= 0 && ordinal < len)
        cell = c.lo[a][k] + ordinal;
      ordinal -= len;
    }
  }
  return cell;
}

/* the term of candidate q (< total) of a particle */
template <int FORM, bool PERIODIC>
static __device__ __forceinline__ double
cmi_sph_candidate_term(const SphMapGeometry &g, const SphCandidates &c,
                       const double p[3], double hi, double reach, int32_t q,
                       const double *__restrict__ values) {
  const int32_t oz = q % c.count[2];
  const int32_t rest = q / c.count[2];
  const int32_t oy = rest % c.count[1];
  const int32_t ox = rest / c.count[1];
  const int32_t i[3] = {cmi_sph_candidate_cell(c, 0, ox),
                        cmi_sph_candidate_cell(c, 1, oy),
                        cmi_sph_candidate_cell(c, 2, oz)};
  double r2 = 0.;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double d = cmi_sph_midpoint(g, a, i[a]) - p[a];
    if (PERIODIC) {
      if (2. * d < -g.box[a])
        d += g.box[a];
      if (2. * d >= g.box[a])
        d -= g.box[a];
    }
    r2 += d * d;
  }
  if (!(r2 < reach * reach))
    return 0.;
  const size_t cell = ((size_t)i[0] * g.ncell[1] + i[1]) * g.ncell[2] + i[2];
  return cmi_sph_shape<FORM>(sqrt(r2), hi) * values[cell];
}

/* ids[m]: the particles of the lane class */
template <int FORM, bool PERIODIC>
__global__ void __launch_bounds__(256)
sph_particles_lane_kernel(SphMapGeometry g, int64_t m,
                          const uint32_t *__restrict__ ids,
                          const double *__restrict__ positions,
                          const double *__restrict__ h,
                          const double *__restrict__ values,
                          double *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m)
    return;
  const size_t i = ids[t];
  const double p[3] = {positions[3 * i], positions[3 * i + 1],
                       positions[3 * i + 2]};
  const double hi = h[i], reach = cmi_sph_reach(FORM, hi);
  SphCandidates c;
  const int32_t total = cmi_sph_candidates(g, p, reach, c);
  double sum = 0.;
  for (int32_t q = 0; q < total; ++q)
    sum += cmi_sph_candidate_term<FORM, PERIODIC>(g, c, p, hi, reach, q,
                                                  values);
  out[i] = sum * (1. / (hi * hi * hi));
}

/* ids[m]: the particles of the wave class, one wave of the 4 of a workgroup
 * each */
template <int FORM, bool PERIODIC>
__global__ void __launch_bounds__(256)
sph_particles_wave_kernel(SphMapGeometry g, int64_t m,
                          const uint32_t *__restrict__ ids,
                          const double *__restrict__ positions,
                          const double *__restrict__ h,
                          const double *__restrict__ values,
                          double *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= m) /* (a whole wave leaves) */
    return;
  const int lane = threadIdx.x & 63;
  const size_t i = ids[t];
  const double p[3] = {positions[3 * i], positions[3 * i + 1],
                       positions[3 * i + 2]};
  const double hi = h[i], reach = cmi_sph_reach(FORM, hi);
  SphCandidates c;
  const int32_t total = cmi_sph_candidates(g, p, reach, c);
  double sum = 0.;
  for (int32_t q = lane; q < total; q += 64)
    sum += cmi_sph_candidate_term<FORM, PERIODIC>(g, c, p, hi, reach, q,
                                                  values);
  /* lanes 0..63 in a fixed tree: 32, 16, ... 1 apart */
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1)
    sum += __shfl_down(sum, step, 64);
  if (lane == 0)
    out[i] = sum * (1. / (hi * hi * hi));
}

#endif /* CMI_SPH_MAP_KERNELS_H */
