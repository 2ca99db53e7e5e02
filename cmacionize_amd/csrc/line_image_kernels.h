/*
 * line_image_kernels.h - emission-line images: ray-traced line-of-sight maps
 * of per-cell emissivities, with dust extinction along the ray. The reference
 * has no such mode (its users sum cells along an axis in Python); this joins
 * the engine's emissivities (device_emissivity.h) to the CCD projection of
 * the dusty mode (dust_pixel, device_dust.h), inverted.
 *
 * Geometry (view angles theta, phi; all of it computed once on the host and
 * passed by value, LineViewDev):
 *   n   = (sin theta cos phi, sin theta sin phi, cos theta)  to the observer
 *   e_x = (-sin phi, cos phi, 0)
 *   e_y = (-cos theta cos phi, -cos theta sin phi, sin theta)
 * Sample (a, b) of pixel (ix, iy) at supersampling s has image coordinates
 *   x = anchor[0] + sides[0] * ((ix + (a + 0.5) / s) / nx),  y likewise,
 * its ray is o + t n with o = x e_x + y e_y, clipped to the box by a slab
 * test: per axis with n != 0, t0 = (lo - o) / n, t1 = (hi - o) / n (as
 * products with 1 / n), t_in = max over axes of min(t0, t1), t_out = min of
 * max(t0, t1); an axis with n == 0 only asks lo <= o < hi. A ray hits if
 * t_in < t_out and both are finite (a NaN coordinate passes through fmax and
 * fmin and leaves them infinite: such a ray misses, it must never reach the
 * march, whose NaN step would advance no index). It starts at o + t_in n,
 * in the cell floor() of that point gives, clamped into the grid, and
 * marches to the box edge with the EXACT marcher's arithmetic
 * (dda_step<false> of device_transport.h at tau =
 * HUGE_VAL: the walls of the cell from its index, the wall distances from
 * the current position, every tying axis advances, DBL_MAX for a zero
 * direction component). line_image_step restates those operations one for
 * one rather than calling dda_step, which loads a 16-B transport record per
 * cell; here the record is the line batch's.
 *
 * Records: {k, s_0 .. s_{L-1}} per cell, fp64, padded to a multiple of 16 B,
 * L <= CMI_LINE_IMAGE_BATCH = 7 (64 B). k is the extinction coefficient
 * (m^-1); with q = j / (4 pi), s = q if k == 0 and q / k otherwise, so that
 * a step of length ds is
 *   k == 0:  I += s ds
 *   else:    dtau = k ds;  I = I exp(-dtau) + s (-expm1(-dtau))
 * without a division in the march. A pixel is the sum of its s^2 samples in
 * the order a outer, b inner, divided by s^2. No atomics anywhere: the same
 * call gives the same bits.
 *
 * Mapping: one lane per sample ray; a wave is an 8 x 8 tile of the sample
 * grid (nx s) x (ny s) and a workgroup of four waves a 16 x 16 tile, so that
 * the rays of a wave form a bundle that crosses the same few cache lines of
 * records at every step (DESIGN.md 4.7 has what was measured and what was
 * not).
 */
#ifndef CMI_LINE_IMAGE_KERNELS_H
#define CMI_LINE_IMAGE_KERNELS_H

#include "device_dust.h"
#include "device_emissivity.h"
#include "device_transport.h"

#define CMI_LINE_IMAGE_BATCH 7
#define CMI_LINE_IMAGE_MAX_SUPERSAMPLE 8
/* sample rays per march launch (bounds the sample buffer of s > 1) */
#define CMI_LINE_IMAGE_LAUNCH_SAMPLES (1ll << 22)
#ifndef CMI_LINE_IMAGE_TILE_X
#define CMI_LINE_IMAGE_TILE_X 8 /* wave tile: TILE_X x (64 / TILE_X) samples */
#endif

struct LineViewDev {
  double n[3], inv_n[3], ex[3], ey[3];
  double img_anchor[2], img_sides[2];
  int32_t nx, ny, s;
  int32_t pad;
};

/* the ray of image coordinates (x, y): false if it misses the box (t_in and
 * t_out are then whatever the slab test left); otherwise the entry point and
 * the cell the march starts in */
__device__ __forceinline__ bool line_image_ray(const GridDev &g,
                                               const LineViewDev &v, double x,
                                               double y, double pos[3],
                                               int32_t index[3], double &t_in,
                                               double &t_out) {
  double o[3];
  t_in = -HUGE_VAL;
  t_out = HUGE_VAL;
  bool hit = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = x * v.ex[a] + y * v.ey[a];
    const double lo = g.anchor[a];
    const double hi = g.anchor[a] + g.box_sides[a];
    if (v.n[a] != 0.) {
      const double t0 = (lo - o[a]) * v.inv_n[a];
      const double t1 = (hi - o[a]) * v.inv_n[a];
      t_in = fmax(t_in, fmin(t0, t1));
      t_out = fmin(t_out, fmax(t0, t1));
    } else {
      hit = hit && (o[a] >= lo && o[a] < hi);
    }
  }
  hit = hit && (t_in < t_out) && t_in > -HUGE_VAL && t_out < HUGE_VAL;
  if (!hit)
    return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pos[a] = o[a] + t_in * v.n[a];
    double c = floor((pos[a] - g.anchor[a]) * g.inv_cellside[a]);
    /* rounding can put the entry point a hair outside the box */
    c = fmin(fmax(c, 0.), (double)(g.ncell[a] - 1));
    index[a] = (int32_t)c;
  }
  return true;
}

/* the geometry of dda_step<false> (device_transport.h) at tau = HUGE_VAL, the
 * same operations in the same order: returns the path length in the cell,
 * moves pos to the wall and index across it */
__device__ __forceinline__ double line_image_step(const GridDev &g,
                                                  const LineViewDev &v,
                                                  double pos[3],
                                                  int32_t index[3]) {
  double d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = g.anchor[a] + g.cellside[a] * (index[a] + g.offset[a]);
    const double hi = lo + g.cellside[a];
    d[a] = (v.n[a] > 0.)
               ? (hi - pos[a]) * v.inv_n[a]
               : ((v.n[a] < 0.) ? (lo - pos[a]) * v.inv_n[a] : DBL_MAX);
  }
  const double ds = fmin(d[0], fmin(d[1], d[2]));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    /* every axis that ties the minimum advances (edges, corners) */
    const int32_t step = (d[a] == ds) ? ((v.n[a] > 0.) ? 1 : -1) : 0;
    pos[a] = pos[a] + ds * v.n[a];
    index[a] += step;
  }
  return ds;
}

__device__ __forceinline__ bool line_image_inside(const GridDev &g,
                                                  const int32_t index[3]) {
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    inside &= (index[a] >= 0 && index[a] < g.ncell[a]);
  return inside;
}

/* one record from a cell's extinction coefficient and its emissivities */
template <int ND>
__device__ __forceinline__ void line_image_store_record(double *rec, double k,
                                                        const double *j,
                                                        int nlines) {
  double r[ND];
  r[0] = k;
#pragma unroll
  for (int l = 0; l < ND - 1; ++l) {
    double s = 0.;
    if (l < nlines) {
      const double q = j[l] / (4. * M_PI);
      s = (k == 0.) ? q : q / k;
    }
    r[1 + l] = s;
  }
  double2 *dst = reinterpret_cast<double2 *>(rec);
#pragma unroll
  for (int h = 0; h < ND / 2; ++h)
    dst[h] = make_double2(r[2 * h], r[2 * h + 1]);
}

struct LineRecordArgs {
  ModelDev model;
  CellsDev cells;
  int64_t ncell;
  int32_t nlines;
  int32_t lines[CMI_LINE_IMAGE_BATCH];
  double dust_cross_section; /* m^2 per hydrogen nucleus */
  double *records;           /* [ncell][ND] */
};

/* records of a batch of emission lines from the cells as they are: k = n_H
 * sigma_dust, j from cell_emissivities */
template <int ND>
__global__ void __launch_bounds__(CMI_BLOCK)
    line_record_kernel(const LineRecordArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    double x[CMI_NION], values[CMI_NEMISSIONLINE];
#pragma unroll
    for (int i = 0; i < CMI_NION; ++i)
      x[i] = a.cells.x[i][c];
    const double ntot = a.cells.number_density[c];
    cell_emissivities(a.model, ntot, a.cells.temperature[c], x, values);
    double j[CMI_LINE_IMAGE_BATCH];
    for (int l = 0; l < CMI_LINE_IMAGE_BATCH; ++l)
      j[l] = l < a.nlines ? values[a.lines[l]] : 0.;
    line_image_store_record<ND>(a.records + c * ND, ntot * a.dust_cross_section,
                                j, a.nlines);
  }
}

/* ---- the cell-luminosity source of the scattered-light images (device_dust.h
 * has the tables' contract and the selection rule) ---- */

struct CellSourceLineArgs {
  ModelDev model;
  CellsDev cells;
  int64_t ncell;
  int32_t line;
  double *weights; /* [ncell] */
};

/* the weights of a line source from the cells as they are: the emissivity of
 * one line (W m^-3), cell_emissivities as emissivity_kernel calls it */
__global__ void __launch_bounds__(CMI_BLOCK)
    cell_source_line_kernel(const CellSourceLineArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    double x[CMI_NION], values[CMI_NEMISSIONLINE];
#pragma unroll
    for (int i = 0; i < CMI_NION; ++i)
      x[i] = a.cells.x[i][c];
    cell_emissivities(a.model, a.cells.number_density[c],
                      a.cells.temperature[c], x, values);
    a.weights[c] = values[a.line];
  }
}

/* the number of weights that are negative or not finite, added to *ninvalid
 * (summed over the wave first, one atomic per wave that found any) */
__global__ void __launch_bounds__(256)
    cell_source_check_kernel(const double *__restrict__ weights, int64_t ncell,
                             unsigned int *ninvalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell;
       c += stride) {
    const double w = weights[c];
    bad += (!(w >= 0.) || w == HUGE_VAL) ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1)
    bad += __shfl_down(bad, off, 64);
  if (threadIdx.x % 64 == 0 && bad)
    atomicAdd(ninvalid, bad);
}

/* C in place of the weights, one thread per block of CMI_CELL_SOURCE_BLOCK
 * cells in cell order - the summation order is the contract -, and the
 * block's total; the running sum B of the totals is the host's pass */
__global__ void __launch_bounds__(64)
    cell_source_block_kernel(double *sums, int64_t ncell, int64_t nblock,
                             double *__restrict__ totals) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblock)
    return;
  const int64_t lo = b * CMI_CELL_SOURCE_BLOCK;
  const int64_t hi =
      (lo + CMI_CELL_SOURCE_BLOCK < ncell) ? lo + CMI_CELL_SOURCE_BLOCK : ncell;
  double sum = 0.;
  for (int64_t c = lo; c < hi; ++c) {
    sum += sums[c];
    sums[c] = sum;
  }
  totals[b] = sum;
}

/* records of a batch of caller-supplied fields ([nfields][ncell] on the
 * device); extinction may be null */
template <int ND>
__global__ void __launch_bounds__(256)
    field_record_kernel(const double *__restrict__ fields,
                        const double *__restrict__ extinction, int64_t ncell,
                        int32_t nfields, double *__restrict__ records) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell)
    return;
  double j[CMI_LINE_IMAGE_BATCH];
#pragma unroll
  for (int l = 0; l < CMI_LINE_IMAGE_BATCH; ++l)
    j[l] = (l < nfields && l < ND - 1) ? fields[(int64_t)l * ncell + c] : 0.;
  line_image_store_record<ND>(records + c * ND, extinction ? extinction[c] : 0.,
                              j, nfields);
}

struct LineMarchArgs {
  GridDev grid;
  LineViewDev view;
  const double *records; /* [ncell][ND] */
  /* sample rows [sx0, sx1) of the sample grid (nx s) x (ny s); sample (sx,
   * sy) of line l goes to out[l * line_stride + (sx - sx0) * ny s + sy] */
  int32_t sx0, sx1;
  int32_t nlines; /* lines of the batch: the record's first nlines sources */
  int64_t line_stride;
  double *out;
};

/* the march: one lane per sample ray, far side to near side */
template <int ND>
__global__ void __launch_bounds__(256)
    line_image_march_kernel(const LineMarchArgs a) {
  constexpr int TX = CMI_LINE_IMAGE_TILE_X, TY = 64 / TX;
  const LineViewDev &v = a.view;
  const int32_t NY = v.ny * v.s;
  /* workgroup: 2 x 2 wave tiles */
  const int32_t tiles_y = (NY + 2 * TY - 1) / (2 * TY);
  const int32_t by = blockIdx.x % tiles_y, bx = blockIdx.x / tiles_y;
  const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t sx = a.sx0 + (2 * bx + (wave >> 1)) * TX + lane / TY;
  const int32_t sy = (2 * by + (wave & 1)) * TY + lane % TY;
  if (sx >= a.sx1 || sy >= NY)
    return;
  const int32_t ix = sx / v.s, iy = sy / v.s;
  const double fa = ((sx - ix * v.s) + 0.5) / v.s;
  const double fb = ((sy - iy * v.s) + 0.5) / v.s;
  const double x = v.img_anchor[0] + v.img_sides[0] * ((ix + fa) / v.nx);
  const double y = v.img_anchor[1] + v.img_sides[1] * ((iy + fb) / v.ny);

  double I[ND - 1];
#pragma unroll
  for (int l = 0; l < ND - 1; ++l)
    I[l] = 0.;
  double pos[3], t_in, t_out;
  int32_t index[3];
  if (line_image_ray(a.grid, v, x, y, pos, index, t_in, t_out)) {
    while (line_image_inside(a.grid, index)) {
      const int64_t cell =
          ((int64_t)index[0] * a.grid.ncell[1] + index[1]) * a.grid.ncell[2] +
          index[2];
      const double2 *rec =
          reinterpret_cast<const double2 *>(a.records + cell * ND);
      double r[ND];
#pragma unroll
      for (int h = 0; h < ND / 2; ++h) {
        const double2 w = rec[h];
        r[2 * h] = w.x;
        r[2 * h + 1] = w.y;
      }
      const double ds = line_image_step(a.grid, v, pos, index);
      const double k = r[0];
      if (k == 0.) {
#pragma unroll
        for (int l = 0; l < ND - 1; ++l)
          I[l] += r[1 + l] * ds;
      } else {
        const double dtau = k * ds;
        const double att = exp(-dtau);
        const double emit = -expm1(-dtau);
#pragma unroll
        for (int l = 0; l < ND - 1; ++l)
          I[l] = I[l] * att + r[1 + l] * emit;
      }
    }
  }
  const int64_t at = (int64_t)(sx - a.sx0) * NY + sy;
  /* (a record of an even number of lines has one padding source) */
#pragma unroll
  for (int l = 0; l < ND - 1; ++l)
    if (l < a.nlines)
      a.out[l * a.line_stride + at] = I[l];
}

/* pixels of rows [ix0, ix1) from their s^2 samples: the sum in the order a
 * outer, b inner, divided by s^2 */
__global__ void __launch_bounds__(256)
    line_image_reduce_kernel(const double *__restrict__ samples,
                             int64_t line_stride, int32_t nlines, int32_t ix0,
                             int32_t ix1, int32_t ny, int32_t s,
                             int64_t npixel, double *__restrict__ image) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)(ix1 - ix0) * ny;
  if (k >= n * nlines)
    return;
  const int32_t l = (int32_t)(k / n);
  const int64_t p = k % n;
  const int32_t rx = (int32_t)(p / ny), iy = (int32_t)(p % ny);
  const int64_t NY = (int64_t)ny * s;
  const double *src = samples + l * line_stride;
  double sum = 0.;
  for (int a = 0; a < s; ++a)
    for (int b = 0; b < s; ++b)
      sum += src[((int64_t)rx * s + a) * NY + (int64_t)iy * s + b];
  image[l * npixel + (int64_t)(ix0 + rx) * ny + iy] = sum / (double)(s * s);
}

/* cmi_gpu_line_image_probe: row k = {t_in, t_out, steps, cells[max_cells],
 * ds[max_cells]} of the ray through image coordinates xy[k] */
__global__ void __launch_bounds__(64)
    line_image_probe_kernel(GridDev g, LineViewDev v,
                            const double *__restrict__ xy, int64_t n,
                            int32_t max_cells, double *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  double *o = out + k * (3 + 2 * (int64_t)max_cells);
  double pos[3], t_in, t_out;
  int32_t index[3];
  if (!line_image_ray(g, v, xy[2 * k], xy[2 * k + 1], pos, index, t_in,
                      t_out)) {
    o[0] = __builtin_nan("");
    o[1] = __builtin_nan("");
    o[2] = 0.;
    return;
  }
  int steps = 0;
  while (line_image_inside(g, index)) {
    const int64_t cell =
        ((int64_t)index[0] * g.ncell[1] + index[1]) * g.ncell[2] + index[2];
    const double ds = line_image_step(g, v, pos, index);
    if (steps < max_cells) {
      o[3 + steps] = (double)cell;
      o[3 + max_cells + steps] = ds;
    }
    ++steps;
  }
  o[0] = t_in;
  o[1] = t_out;
  o[2] = (double)steps;
}

#endif
