/*
 * line_cube_reference.c - CPU restatement of the spectral line cubes
 * (include/cmi_gpu.h, "spectral line cubes") in plain C, written from the
 * contract and not from the kernels. The ray geometry (set_view, enter,
 * inside, step) is copied from line_image_reference.c, so that cells and
 * path lengths are the images'.
 *
 * Built by tests/line_cube_lib.py with gcc -O2 -ffp-contract=off -fopenmp,
 * so that every product and sum below is one IEEE operation, as on the
 * device.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  /* the box and its grid */
  double anchor[3], sides[3], cell[3], inv_cell[3];
  int32_t ncell[3];
  /* the view: to the observer, the image axes */
  double n[3], inv_n[3], ex[3], ey[3];
} View;

static void set_view(View *v, const double *anchor, const double *sides,
                     const int32_t *ncell, double theta, double phi) {
  for (int a = 0; a < 3; ++a) {
    v->anchor[a] = anchor[a];
    v->sides[a] = sides[a];
    v->ncell[a] = ncell[a];
    v->cell[a] = sides[a] / ncell[a];
    v->inv_cell[a] = 1. / v->cell[a];
  }
  const double st = sin(theta), ct = cos(theta);
  const double sp = sin(phi), cp = cos(phi);
  v->n[0] = st * cp;
  v->n[1] = st * sp;
  v->n[2] = ct;
  v->ex[0] = -sp;
  v->ex[1] = cp;
  v->ex[2] = 0.;
  v->ey[0] = -ct * cp;
  v->ey[1] = -ct * sp;
  v->ey[2] = st;
  for (int a = 0; a < 3; ++a)
    v->inv_n[a] = 1. / v->n[a];
}

/* the slab test and the entry cell; 0 = the ray misses the box. A ray whose
 * entry or exit is not finite (a NaN coordinate leaves them at their initial
 * infinities) misses too. */
static int enter(const View *v, double x, double y, double pos[3],
                 int32_t idx[3], double *t_in, double *t_out) {
  double o[3];
  double tin = -HUGE_VAL, tout = HUGE_VAL;
  int hit = 1;
  for (int a = 0; a < 3; ++a) {
    o[a] = x * v->ex[a] + y * v->ey[a];
    const double lo = v->anchor[a];
    const double hi = v->anchor[a] + v->sides[a];
    if (v->n[a] != 0.) {
      const double t0 = (lo - o[a]) * v->inv_n[a];
      const double t1 = (hi - o[a]) * v->inv_n[a];
      tin = fmax(tin, fmin(t0, t1));
      tout = fmin(tout, fmax(t0, t1));
    } else if (!(o[a] >= lo && o[a] < hi)) {
      hit = 0;
    }
  }
  *t_in = tin;
  *t_out = tout;
  if (!hit || !(tin < tout) || !(tin > -HUGE_VAL) || !(tout < HUGE_VAL))
    return 0;
  for (int a = 0; a < 3; ++a) {
    pos[a] = o[a] + tin * v->n[a];
    double c = floor((pos[a] - v->anchor[a]) * v->inv_cell[a]);
    if (c < 0.)
      c = 0.;
    if (c > (double)(v->ncell[a] - 1))
      c = (double)(v->ncell[a] - 1);
    idx[a] = (int32_t)c;
  }
  return 1;
}

static int inside(const View *v, const int32_t idx[3]) {
  for (int a = 0; a < 3; ++a)
    if (idx[a] < 0 || idx[a] >= v->ncell[a])
      return 0;
  return 1;
}

/* one cell crossing of the exact marcher: the walls of the cell from its
 * index, the distances to them from the current position, every tying axis
 * advances */
static double step(const View *v, double pos[3], int32_t idx[3]) {
  double d[3];
  for (int a = 0; a < 3; ++a) {
    const double lo = v->anchor[a] + v->cell[a] * idx[a];
    const double hi = lo + v->cell[a];
    if (v->n[a] > 0.)
      d[a] = (hi - pos[a]) * v->inv_n[a];
    else if (v->n[a] < 0.)
      d[a] = (lo - pos[a]) * v->inv_n[a];
    else
      d[a] = DBL_MAX;
  }
  const double ds = fmin(d[0], fmin(d[1], d[2]));
  for (int a = 0; a < 3; ++a) {
    if (d[a] == ds)
      idx[a] += (v->n[a] > 0.) ? 1 : -1;
    pos[a] = pos[a] + ds * v->n[a];
  }
  return ds;
}

/* the clamped error function of the contract for the edge at distance d = e
 * - u from the line centre, width b; b == 0: the step function with the
 * lower edge inclusive (an edge at u counts as below it) */
static double clamped_erf(double d, double b) {
  if (b == 0.)
    return d > 0. ? 1. : -1.;
  const double z = d / b;
  if (z >= 6.)
    return 1.;
  if (z <= -6.)
    return -1.;
  return erf(z);
}

/* cube[(l * nchan + c) * nx * ny + pixel] of the per-cell sources
 * j[nl][ncells] with the widths b[nl][ncells], the extinction coefficients
 * k[ncells] (NULL: none) and the velocities vel[3][ncells] (NULL: at rest);
 * returns the number of cell crossings */
int64_t cref_render(const double *anchor, const double *sides,
                    const int32_t *ncell, double theta, double phi,
                    int32_t nx, int32_t ny, const double *img_anchor,
                    const double *img_sides, int32_t s, int32_t nl,
                    const double *j, const double *b, const double *k,
                    const double *vel, int32_t nchan, double vmin,
                    double vmax, double *cube) {
  View v;
  set_view(&v, anchor, sides, ncell, theta, phi);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  const int64_t npixel = (int64_t)nx * ny;
  const double dv = (vmax - vmin) / nchan;
  double *edge = malloc(sizeof(double) * ((size_t)nchan + 1));
  for (int c = 0; c <= nchan; ++c)
    edge[c] = vmin + c * dv;
  /* the radial velocity per cell, positive for matter that recedes */
  double *u = malloc(sizeof(double) * (size_t)ncells);
  for (int64_t i = 0; i < ncells; ++i)
    u[i] = vel ? -((vel[i] * v.n[0] + vel[ncells + i] * v.n[1]) +
                   vel[2 * ncells + i] * v.n[2])
               : 0.;
  int64_t crossings = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : crossings)
  for (int64_t pixel = 0; pixel < npixel; ++pixel) {
    const int32_t ix = (int32_t)(pixel / ny), iy = (int32_t)(pixel % ny);
    double *I = malloc(sizeof(double) * 2 * (size_t)nchan);
    double *sum = I + nchan;
    for (int l = 0; l < nl; ++l) {
      const double *jl = j + l * ncells, *bl = b + l * ncells;
      for (int c = 0; c < nchan; ++c)
        sum[c] = 0.;
      for (int sa = 0; sa < s; ++sa)
        for (int sb = 0; sb < s; ++sb) {
          const double fa = (sa + 0.5) / s;
          const double fb = (sb + 0.5) / s;
          const double x = img_anchor[0] + img_sides[0] * ((ix + fa) / nx);
          const double y = img_anchor[1] + img_sides[1] * ((iy + fb) / ny);
          for (int c = 0; c < nchan; ++c)
            I[c] = 0.;
          double pos[3], t_in, t_out;
          int32_t idx[3];
          if (enter(&v, x, y, pos, idx, &t_in, &t_out)) {
            while (inside(&v, idx)) {
              const int64_t cell =
                  ((int64_t)idx[0] * v.ncell[1] + idx[1]) * v.ncell[2] +
                  idx[2];
              const double ds = step(&v, pos, idx);
              if (l == 0)
                ++crossings;
              const double kc = k ? k[cell] : 0.;
              const double q = jl[cell] / (4. * M_PI);
              double att = 1., w;
              if (kc == 0.) {
                w = q * ds;
              } else {
                const double dtau = kc * ds;
                att = exp(-dtau);
                w = (q / kc) * -expm1(-dtau);
              }
              double E_lo = clamped_erf(edge[0] - u[cell], bl[cell]);
              for (int c = 0; c < nchan; ++c) {
                const double E_hi =
                    clamped_erf(edge[c + 1] - u[cell], bl[cell]);
                const double f = 0.5 * (E_hi - E_lo);
                if (kc == 0.)
                  I[c] += w * f;
                else
                  I[c] = I[c] * att + w * f;
                E_lo = E_hi;
              }
            }
          }
          for (int c = 0; c < nchan; ++c)
            sum[c] += I[c];
        }
      for (int c = 0; c < nchan; ++c)
        cube[((int64_t)l * nchan + c) * npixel + pixel] =
            sum[c] / (double)(s * s);
    }
    free(I);
  }
  free(u);
  free(edge);
  return crossings;
}
