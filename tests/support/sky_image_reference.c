/*
 * sky_image_reference.c - CPU restatement of the sky maps (include/cmi_gpu.h,
 * "sky maps"), written from the description of the mode, not from the
 * kernels: rays from one origin in directions of their own, the probe rows,
 * and the intensities of given per-cell quantities {k, j_0 .. j_{L-1}},
 * integrated from the observer outwards.
 *
 * Built by tests/sky_image_lib.py with gcc -O2 -ffp-contract=off -fopenmp, so
 * that every product and sum below is one IEEE operation, as on the device.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  double anchor[3], sides[3], cell[3], inv_cell[3];
  int32_t ncell[3];
  double o[3];
} Scene;

typedef struct {
  double d[3], inv_d[3];
} Ray;

static void set_scene(Scene *s, const double *anchor, const double *sides,
                      const int32_t *ncell, const double *origin) {
  for (int a = 0; a < 3; ++a) {
    s->anchor[a] = anchor[a];
    s->sides[a] = sides[a];
    s->ncell[a] = ncell[a];
    s->cell[a] = sides[a] / ncell[a];
    s->inv_cell[a] = 1. / s->cell[a];
    s->o[a] = origin[a];
  }
}

static void set_ray(Ray *r, const double *d) {
  for (int a = 0; a < 3; ++a) {
    r->d[a] = d[a];
    r->inv_d[a] = 1. / d[a];
  }
}

/* the slab test and the start: 0 = the ray misses the box */
static int start(const Scene *s, const Ray *r, double pos[3], int32_t idx[3],
                 double *t_start, double *t_out) {
  double tin = -HUGE_VAL, tout = HUGE_VAL;
  int hit = 1;
  for (int a = 0; a < 3; ++a) {
    const double lo = s->anchor[a];
    const double hi = s->anchor[a] + s->sides[a];
    if (r->d[a] != 0.) {
      const double t0 = (lo - s->o[a]) * r->inv_d[a];
      const double t1 = (hi - s->o[a]) * r->inv_d[a];
      tin = fmax(tin, fmin(t0, t1));
      tout = fmin(tout, fmax(t0, t1));
    } else if (!(s->o[a] >= lo && s->o[a] < hi)) {
      hit = 0;
    }
  }
  const double ts = (tin > 0.) ? tin : 0.;
  *t_start = ts;
  *t_out = tout;
  if (!hit || !(ts < tout) || !(tout < HUGE_VAL))
    return 0;
  for (int a = 0; a < 3; ++a) {
    /* inside the box the march starts at the origin itself */
    pos[a] = (tin > 0.) ? s->o[a] + tin * r->d[a] : s->o[a];
    double c = floor((pos[a] - s->anchor[a]) * s->inv_cell[a]);
    if (c < 0.)
      c = 0.;
    if (c > (double)(s->ncell[a] - 1))
      c = (double)(s->ncell[a] - 1);
    idx[a] = (int32_t)c;
  }
  return 1;
}

static int inside(const Scene *s, const int32_t idx[3]) {
  for (int a = 0; a < 3; ++a)
    if (idx[a] < 0 || idx[a] >= s->ncell[a])
      return 0;
  return 1;
}

/* one cell crossing of the exact marcher: the walls of the cell from its
 * index, the distances to them from the current position, every tying axis
 * advances */
static double step(const Scene *s, const Ray *r, double pos[3],
                   int32_t idx[3]) {
  double d[3];
  for (int a = 0; a < 3; ++a) {
    const double lo = s->anchor[a] + s->cell[a] * idx[a];
    const double hi = lo + s->cell[a];
    if (r->d[a] > 0.)
      d[a] = (hi - pos[a]) * r->inv_d[a];
    else if (r->d[a] < 0.)
      d[a] = (lo - pos[a]) * r->inv_d[a];
    else
      d[a] = DBL_MAX;
  }
  const double ds = fmin(d[0], fmin(d[1], d[2]));
  for (int a = 0; a < 3; ++a) {
    if (d[a] == ds)
      idx[a] += (r->d[a] > 0.) ? 1 : -1;
    pos[a] = pos[a] + ds * r->d[a];
  }
  return ds;
}

/* rows {t_start, t_out, steps, cells[max_cells], ds[max_cells]} of the rays
 * from origin in directions[n][3] */
void sref_probe(const double *anchor, const double *sides,
                const int32_t *ncell, const double *origin, int64_t n,
                const double *directions, int32_t max_cells, double *out) {
  Scene s;
  set_scene(&s, anchor, sides, ncell, origin);
  const int64_t width = 3 + 2 * (int64_t)max_cells;
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t k = 0; k < n; ++k) {
    double *o = out + k * width;
    memset(o, 0, sizeof(double) * width);
    Ray r;
    set_ray(&r, directions + 3 * k);
    double pos[3], t_start, t_out;
    int32_t idx[3];
    if (!start(&s, &r, pos, idx, &t_start, &t_out)) {
      o[0] = NAN;
      o[1] = NAN;
      continue;
    }
    int steps = 0;
    while (inside(&s, idx)) {
      const int64_t cell =
          ((int64_t)idx[0] * s.ncell[1] + idx[1]) * s.ncell[2] + idx[2];
      const double ds = step(&s, &r, pos, idx);
      if (steps < max_cells) {
        o[3 + steps] = (double)cell;
        o[3 + max_cells + steps] = ds;
      }
      ++steps;
    }
    o[0] = t_start;
    o[1] = t_out;
    o[2] = (double)steps;
  }
}

/* out[l][n] of the per-cell quantities j[nl][ncells] (nl <= 64) with the
 * extinction coefficients k[ncells] (NULL: none); returns the number of cell
 * crossings */
int64_t sref_render(const double *anchor, const double *sides,
                    const int32_t *ncell, const double *origin, int64_t n,
                    const double *directions, int32_t nl, const double *j,
                    const double *k, double *out) {
  Scene s;
  set_scene(&s, anchor, sides, ncell, origin);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  /* the source term per steradian, j / 4 pi, once per cell; over k where
   * there is dust */
  double *q = malloc(sizeof(double) * (size_t)nl * (size_t)ncells);
  for (int l = 0; l < nl; ++l)
    for (int64_t c = 0; c < ncells; ++c) {
      const double v = j[l * ncells + c] / (4. * M_PI);
      q[l * ncells + c] = (k && k[c] != 0.) ? v / k[c] : v;
    }
  int64_t crossings = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : crossings)
  for (int64_t ray = 0; ray < n; ++ray) {
    Ray r;
    set_ray(&r, directions + 3 * ray);
    double I[64];
    for (int l = 0; l < nl; ++l)
      I[l] = 0.;
    double T = 1.;
    double pos[3], t_start, t_out;
    int32_t idx[3];
    if (start(&s, &r, pos, idx, &t_start, &t_out)) {
      while (inside(&s, idx)) {
        const int64_t cell =
            ((int64_t)idx[0] * s.ncell[1] + idx[1]) * s.ncell[2] + idx[2];
        const double ds = step(&s, &r, pos, idx);
        ++crossings;
        const double kc = k ? k[cell] : 0.;
        if (kc == 0.) {
          for (int l = 0; l < nl; ++l)
            I[l] += T * (q[l * ncells + cell] * ds);
        } else {
          const double dtau = kc * ds;
          const double att = exp(-dtau);
          const double emit = -expm1(-dtau);
          for (int l = 0; l < nl; ++l)
            I[l] += T * (q[l * ncells + cell] * emit);
          T = T * att;
        }
      }
    }
    for (int l = 0; l < nl; ++l)
      out[l * n + ray] = I[l];
  }
  free(q);
  return crossings;
}
