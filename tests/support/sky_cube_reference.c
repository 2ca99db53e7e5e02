/*
 * sky_cube_reference.c - CPU restatement of the sky cubes (include/cmi_gpu.h,
 * "sky cubes") in plain C, written from the contract and not from the
 * kernels. The ray geometry (set_scene, set_ray, start, inside, step) is
 * copied from sky_image_reference.c, so that cells and path lengths are the
 * sky maps'; the channel fractions are spelt out from "spectral line cubes",
 * b == 0 as a case of its own.
 *
 * Built by tests/sky_cube_lib.py with gcc -O2 -ffp-contract=off -fopenmp, so
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
static int start(const Scene *s, const Ray *r, double pos[3], int32_t idx[3]) {
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

/* one cell crossing of the exact marcher */
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

/* E((e - u) / b) of the contract from d = e - u; b == 0 is the step function
 * with the lower edge inclusive: an edge at u counts as below it */
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

/* out[(l * nchan + c) * n + ray] of the per-cell sources j[nl][ncells] with
 * the widths b[nl][ncells], the extinction coefficients k[ncells] (NULL:
 * none), the velocities vel[3][ncells] (NULL: at rest) and the observer's
 * velocity v_obs[3] (NULL: at rest); returns the number of cell crossings */
int64_t scref_render(const double *anchor, const double *sides,
                     const int32_t *ncell, const double *origin,
                     const double *v_obs, int64_t n, const double *directions,
                     int32_t nl, const double *j, const double *b,
                     const double *k, const double *vel, int32_t nchan,
                     double vmin, double vmax, double *out) {
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
  /* the velocity relative to the observer, once per cell */
  double *w = malloc(sizeof(double) * 3 * (size_t)ncells);
  for (int a = 0; a < 3; ++a)
    for (int64_t c = 0; c < ncells; ++c)
      w[a * ncells + c] =
          (vel ? vel[a * ncells + c] : 0.) - (v_obs ? v_obs[a] : 0.);
  const double dv = (vmax - vmin) / nchan;
  double *edge = malloc(sizeof(double) * ((size_t)nchan + 1));
  for (int c = 0; c <= nchan; ++c)
    edge[c] = vmin + (double)c * dv;
  int64_t crossings = 0;
#pragma omp parallel reduction(+ : crossings)
  {
    double *I = malloc(sizeof(double) * (size_t)nchan);
#pragma omp for schedule(dynamic, 16)
    for (int64_t ray = 0; ray < n; ++ray) {
      Ray r;
      set_ray(&r, directions + 3 * ray);
      for (int l = 0; l < nl; ++l) {
        for (int c = 0; c < nchan; ++c)
          I[c] = 0.;
        double T = 1.;
        double pos[3];
        int32_t idx[3];
        if (start(&s, &r, pos, idx)) {
          while (inside(&s, idx)) {
            const int64_t cell =
                ((int64_t)idx[0] * s.ncell[1] + idx[1]) * s.ncell[2] + idx[2];
            const double ds = step(&s, &r, pos, idx);
            if (l == 0)
              ++crossings;
            /* d points away from the observer: positive u recedes */
            const double u = (w[cell] * r.d[0] + w[ncells + cell] * r.d[1]) +
                             w[2 * ncells + cell] * r.d[2];
            const double kc = k ? k[cell] : 0.;
            const double sc = q[l * ncells + cell];
            const double bc = b[l * ncells + cell];
            double att = 1., emitted;
            if (kc == 0.) {
              emitted = sc * ds;
            } else {
              const double dtau = kc * ds;
              att = exp(-dtau);
              emitted = sc * -expm1(-dtau);
            }
            double E_lo = clamped_erf(edge[0] - u, bc);
            for (int c = 0; c < nchan; ++c) {
              const double E_hi = clamped_erf(edge[c + 1] - u, bc);
              const double f = 0.5 * (E_hi - E_lo);
              I[c] += T * (emitted * f);
              E_lo = E_hi;
            }
            if (kc != 0.)
              T = T * att;
          }
        }
        for (int c = 0; c < nchan; ++c)
          out[((int64_t)l * nchan + c) * n + ray] = I[c];
      }
    }
    free(I);
  }
  free(q);
  free(w);
  free(edge);
  return crossings;
}
