/*
 * line_image_kernels.h - emission-line images: ray-traced line-of-sight maps
 * of per-cell emissivities, with dust extinction along the ray. The reference
 * has no such mode (its users sum cells along an axis in Python); this joins
 * the engine's emissivities (device_emissivity.h) to the CCD projection of
 * the dusty mode (dust_pixel, device_dust.h), inverted.
 *
 * The rays, their cells and the path lengths are ray_walk.h's (GridRay with
 * the parallel camera's start, tile_sample): one direction n for all rays, the
 * march runs from the far side of the box to the near one.
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
 */
#ifndef CMI_LINE_IMAGE_KERNELS_H
#define CMI_LINE_IMAGE_KERNELS_H

#include "device_dust.h"
#include "device_emissivity.h"
#include "device_transport.h"
#include "ray_walk.h"

#define CMI_LINE_IMAGE_BATCH 7
#define CMI_LINE_IMAGE_MAX_SUPERSAMPLE 8
/* sample rays per march launch (bounds the sample buffer of s > 1) */
#define CMI_LINE_IMAGE_LAUNCH_SAMPLES (1ll << 22)

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
  int32_t sx, sy;
  double x, y;
  if (!tile_sample(a.view, a.sx0, a.sx1, sx, sy, x, y))
    return;

  double I[ND - 1];
#pragma unroll
  for (int l = 0; l < ND - 1; ++l)
    I[l] = 0.;
  GridRay ray;
  if (ray.start(a.grid, a.view, x, y)) {
    while (ray.inside(a.grid)) {
      const double2 *rec = reinterpret_cast<const double2 *>(
          a.records + ray.cell(a.grid) * ND);
      double r[ND];
#pragma unroll
      for (int h = 0; h < ND / 2; ++h) {
        const double2 w = rec[h];
        r[2 * h] = w.x;
        r[2 * h + 1] = w.y;
      }
      const double ds = ray.step(a.grid);
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
  const int64_t at = tile_sample_at(a.view, a.sx0, sx, sy);
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
  GridRay ray;
  const bool hit = ray.start(g, v, xy[2 * k], xy[2 * k + 1]);
  probe_row(g, ray, hit, max_cells, o, [](int64_t, double, int) {});
}

#endif
