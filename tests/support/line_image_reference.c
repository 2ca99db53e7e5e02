/*
 * line_image_reference.c - CPU restatement of the emission-line images
 * (include/cmi_gpu.h, "emission-line images"), written from the description
 * of the mode, not from the kernels: the ray geometry with its probe rows,
 * and the images of given per-cell quantities {k, j_0 .. j_{L-1}}.
 *
 * Built by tests/line_image_lib.py with gcc -O2 -ffp-contract=off -fopenmp,
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

/* rows {t_in, t_out, steps, cells[max_cells], ds[max_cells]} of the rays
 * through xy[n][2] */
void lref_probe(const double *anchor, const double *sides,
                const int32_t *ncell, double theta, double phi, int64_t n,
                const double *xy, int32_t max_cells, double *out) {
  View v;
  set_view(&v, anchor, sides, ncell, theta, phi);
  const int64_t width = 3 + 2 * (int64_t)max_cells;
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t k = 0; k < n; ++k) {
    double *o = out + k * width;
    memset(o, 0, sizeof(double) * width);
    double pos[3], t_in, t_out;
    int32_t idx[3];
    if (!enter(&v, xy[2 * k], xy[2 * k + 1], pos, idx, &t_in, &t_out)) {
      o[0] = NAN;
      o[1] = NAN;
      continue;
    }
    int steps = 0;
    while (inside(&v, idx)) {
      const int64_t cell =
          ((int64_t)idx[0] * v.ncell[1] + idx[1]) * v.ncell[2] + idx[2];
      const double ds = step(&v, pos, idx);
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
}

/* images[l][nx * ny] of the per-cell quantities j[nl][ncells] with the
 * extinction coefficients k[ncells] (NULL: none); returns the number of cell
 * crossings */
int64_t lref_render(const double *anchor, const double *sides,
                    const int32_t *ncell, double theta, double phi,
                    int32_t nx, int32_t ny, const double *img_anchor,
                    const double *img_sides, int32_t s, int32_t nl,
                    const double *j, const double *k, double *images) {
  View v;
  set_view(&v, anchor, sides, ncell, theta, phi);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  const int64_t npixel = (int64_t)nx * ny;
  /* the source term per steradian, j / 4 pi, once per cell */
  double *q = malloc(sizeof(double) * (size_t)nl * (size_t)ncells);
  for (int64_t i = 0; i < (int64_t)nl * ncells; ++i)
    q[i] = j[i] / (4. * M_PI);
  int64_t crossings = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : crossings)
  for (int64_t pixel = 0; pixel < npixel; ++pixel) {
    const int32_t ix = (int32_t)(pixel / ny), iy = (int32_t)(pixel % ny);
    double sum[64];
    double I[64];
    for (int l = 0; l < nl; ++l)
      sum[l] = 0.;
    for (int a = 0; a < s; ++a)
      for (int b = 0; b < s; ++b) {
        const double fa = (a + 0.5) / s;
        const double fb = (b + 0.5) / s;
        const double x = img_anchor[0] + img_sides[0] * ((ix + fa) / nx);
        const double y = img_anchor[1] + img_sides[1] * ((iy + fb) / ny);
        for (int l = 0; l < nl; ++l)
          I[l] = 0.;
        double pos[3], t_in, t_out;
        int32_t idx[3];
        if (enter(&v, x, y, pos, idx, &t_in, &t_out)) {
          while (inside(&v, idx)) {
            const int64_t cell =
                ((int64_t)idx[0] * v.ncell[1] + idx[1]) * v.ncell[2] + idx[2];
            const double ds = step(&v, pos, idx);
            ++crossings;
            const double kc = k ? k[cell] : 0.;
            if (kc == 0.) {
              for (int l = 0; l < nl; ++l)
                I[l] += q[l * ncells + cell] * ds;
            } else {
              const double dtau = kc * ds;
              const double att = exp(-dtau);
              const double emit = -expm1(-dtau);
              for (int l = 0; l < nl; ++l)
                I[l] = I[l] * att + (q[l * ncells + cell] / kc) * emit;
            }
          }
        }
        for (int l = 0; l < nl; ++l)
          sum[l] += I[l];
      }
    for (int l = 0; l < nl; ++l)
      images[l * npixel + pixel] = sum[l] / (double)(s * s);
  }
  free(q);
  return crossings;
}
