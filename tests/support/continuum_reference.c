/*
 * continuum_reference.c - CPU restatement of the continuum images
 * (include/cmi_gpu.h, "continuum images") in plain C, written from the
 * contract and not from the kernels: the parallel camera's rays and the rays
 * from a point through a box of cells, and the formal solution with a
 * per-cell, per-channel absorption coefficient and source function along
 * them.
 *
 * Built by tests/continuum_lib.py with gcc -O2 -ffp-contract=off -fopenmp, so
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
} Grid;

/* a ray o + t d with 1 / d per component */
typedef struct {
  double o[3], d[3], inv_d[3];
} Ray;

static void set_grid(Grid *g, const double *anchor, const double *sides,
                     const int32_t *ncell) {
  for (int a = 0; a < 3; ++a) {
    g->anchor[a] = anchor[a];
    g->sides[a] = sides[a];
    g->ncell[a] = ncell[a];
    g->cell[a] = sides[a] / ncell[a];
    g->inv_cell[a] = 1. / g->cell[a];
  }
}

/* the parallel camera: n to the observer and the image axes */
typedef struct {
  double n[3], ex[3], ey[3];
} Camera;

static void set_camera(Camera *c, double theta, double phi) {
  const double st = sin(theta), ct = cos(theta);
  const double sp = sin(phi), cp = cos(phi);
  c->n[0] = st * cp;
  c->n[1] = st * sp;
  c->n[2] = ct;
  c->ex[0] = -sp;
  c->ex[1] = cp;
  c->ex[2] = 0.;
  c->ey[0] = -ct * cp;
  c->ey[1] = -ct * sp;
  c->ey[2] = st;
}

/* the ray of the image coordinates (x, y): it starts in the image plane and
 * runs towards the observer, so that the march goes from the far side to the
 * near side */
static void camera_ray(const Camera *c, double x, double y, Ray *r) {
  for (int a = 0; a < 3; ++a) {
    r->o[a] = x * c->ex[a] + y * c->ey[a];
    r->d[a] = c->n[a];
    r->inv_d[a] = 1. / c->n[a];
  }
}

static void point_ray(const double *origin, const double *d, Ray *r) {
  for (int a = 0; a < 3; ++a) {
    r->o[a] = origin[a];
    r->d[a] = d[a];
    r->inv_d[a] = 1. / d[a];
  }
}

/* the slab test and the first cell; 0 = the ray misses the box. from_point:
 * the ray starts at its origin (t >= 0), otherwise it is a whole line. */
static int enter(const Grid *g, const Ray *r, int from_point, double pos[3],
                 int32_t idx[3], double *t0, double *t1) {
  double tin = -HUGE_VAL, tout = HUGE_VAL;
  int hit = 1;
  for (int a = 0; a < 3; ++a) {
    const double lo = g->anchor[a];
    const double hi = g->anchor[a] + g->sides[a];
    if (r->d[a] != 0.) {
      const double ta = (lo - r->o[a]) * r->inv_d[a];
      const double tb = (hi - r->o[a]) * r->inv_d[a];
      tin = fmax(tin, fmin(ta, tb));
      tout = fmin(tout, fmax(ta, tb));
    } else if (!(r->o[a] >= lo && r->o[a] < hi)) {
      hit = 0;
    }
  }
  int at_origin = 0;
  if (from_point) {
    at_origin = !(tin > 0.);
    const double ts = at_origin ? 0. : tin;
    *t0 = ts;
    *t1 = tout;
    if (!hit || !(ts < tout) || !(tout < HUGE_VAL))
      return 0;
  } else {
    *t0 = tin;
    *t1 = tout;
    if (!hit || !(tin < tout) || !(tin > -HUGE_VAL) || !(tout < HUGE_VAL))
      return 0;
  }
  for (int a = 0; a < 3; ++a) {
    pos[a] = at_origin ? r->o[a] : r->o[a] + tin * r->d[a];
    double c = floor((pos[a] - g->anchor[a]) * g->inv_cell[a]);
    if (c < 0.)
      c = 0.;
    if (c > (double)(g->ncell[a] - 1))
      c = (double)(g->ncell[a] - 1);
    idx[a] = (int32_t)c;
  }
  return 1;
}

static int inside(const Grid *g, const int32_t idx[3]) {
  for (int a = 0; a < 3; ++a)
    if (idx[a] < 0 || idx[a] >= g->ncell[a])
      return 0;
  return 1;
}

/* one cell crossing: the walls of the cell from its index, the distances to
 * them from the current position, every tying axis advances */
static double step(const Grid *g, const Ray *r, double pos[3],
                   int32_t idx[3]) {
  double d[3];
  for (int a = 0; a < 3; ++a) {
    const double lo = g->anchor[a] + g->cell[a] * idx[a];
    const double hi = lo + g->cell[a];
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

static int64_t cell_of(const Grid *g, const int32_t idx[3]) {
  return ((int64_t)idx[0] * g->ncell[1] + idx[1]) * g->ncell[2] + idx[2];
}

/* both integrations of the contract for the nf channels of one ray; I[nf]
 * and T[nf] are the caller's. Optional trace (max_cells > 0): cells, ds and
 * I[f][i] after step i. Returns the number of crossings. */
static int integrate(const Grid *g, const Ray *r, int from_point, int32_t nf,
                     int64_t ncells, const double *kappa,
                     const double *source, const double *bg, double *I,
                     double *T, double *t0, double *t1, int *hit_out,
                     int32_t max_cells, double *cells, double *dss,
                     double *I_steps) {
  for (int f = 0; f < nf; ++f) {
    I[f] = from_point ? 0. : (bg ? bg[f] : 0.);
    T[f] = 1.;
  }
  double pos[3];
  int32_t idx[3];
  int steps = 0;
  const int hit = enter(g, r, from_point, pos, idx, t0, t1);
  if (hit_out)
    *hit_out = hit;
  if (hit) {
    while (inside(g, idx)) {
      const int64_t cell = cell_of(g, idx);
      const double ds = step(g, r, pos, idx);
      for (int f = 0; f < nf; ++f) {
        const double k = kappa[f * ncells + cell];
        const double S = source[f * ncells + cell];
        const double em = expm1(-(k * ds));
        if (from_point) {
          I[f] = I[f] + T[f] * (S * -em);
          T[f] = T[f] + T[f] * em;
        } else {
          I[f] = I[f] + em * (I[f] - S);
        }
        if (steps < max_cells)
          I_steps[(int64_t)f * max_cells + steps] = I[f];
      }
      if (steps < max_cells) {
        cells[steps] = (double)cell;
        dss[steps] = ds;
      }
      ++steps;
    }
  }
  if (from_point)
    for (int f = 0; f < nf; ++f)
      I[f] = I[f] + T[f] * (bg ? bg[f] : 0.);
  return steps;
}

/* out[f][nx * ny] of the parallel camera; returns the largest number of
 * crossings of a sample ray */
int64_t kref_images(const double *anchor, const double *sides,
                    const int32_t *ncell, double theta, double phi,
                    int32_t nx, int32_t ny, const double *img_anchor,
                    const double *img_sides, int32_t s, int32_t nf,
                    const double *kappa, const double *source,
                    const double *bg, double *out) {
  Grid g;
  Camera cam;
  set_grid(&g, anchor, sides, ncell);
  set_camera(&cam, theta, phi);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  const int64_t npixel = (int64_t)nx * ny;
  int64_t longest = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(max : longest)
  for (int64_t pixel = 0; pixel < npixel; ++pixel) {
    const int32_t ix = (int32_t)(pixel / ny), iy = (int32_t)(pixel % ny);
    double *I = malloc(sizeof(double) * 3 * (size_t)nf);
    double *T = I + nf, *sum = T + nf;
    for (int f = 0; f < nf; ++f)
      sum[f] = 0.;
    for (int sa = 0; sa < s; ++sa)
      for (int sb = 0; sb < s; ++sb) {
        const double fa = (sa + 0.5) / s;
        const double fb = (sb + 0.5) / s;
        const double x = img_anchor[0] + img_sides[0] * ((ix + fa) / nx);
        const double y = img_anchor[1] + img_sides[1] * ((iy + fb) / ny);
        Ray r;
        camera_ray(&cam, x, y, &r);
        double t0, t1;
        const int steps = integrate(&g, &r, 0, nf, ncells, kappa, source, bg,
                                    I, T, &t0, &t1, NULL, 0, NULL, NULL, NULL);
        if (steps > longest)
          longest = steps;
        for (int f = 0; f < nf; ++f)
          sum[f] += I[f];
      }
    for (int f = 0; f < nf; ++f)
      out[f * npixel + pixel] = sum[f] / (double)(s * s);
    free(I);
  }
  return longest;
}

/* out[f][n] of the rays from origin along directions[n][3]; returns the
 * largest number of crossings of a ray */
int64_t kref_sky(const double *anchor, const double *sides,
                 const int32_t *ncell, const double *origin, int64_t n,
                 const double *directions, int32_t nf, const double *kappa,
                 const double *source, const double *bg, double *out) {
  Grid g;
  set_grid(&g, anchor, sides, ncell);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  int64_t longest = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(max : longest)
  for (int64_t k = 0; k < n; ++k) {
    double *I = malloc(sizeof(double) * 2 * (size_t)nf);
    double *T = I + nf;
    Ray r;
    point_ray(origin, directions + 3 * k, &r);
    double t0, t1;
    const int steps = integrate(&g, &r, 1, nf, ncells, kappa, source, bg, I,
                                T, &t0, &t1, NULL, 0, NULL, NULL, NULL);
    if (steps > longest)
      longest = steps;
    for (int f = 0; f < nf; ++f)
      out[f * n + k] = I[f];
    free(I);
  }
  return longest;
}

/* rows {t0, t1, steps, cells[max_cells], ds[max_cells], I[nf][max_cells],
 * I_end[nf]}: point == 0, view = {theta, phi}, rays[n][2]; point == 1, view =
 * the origin, rays[n][3] */
void kref_probe(const double *anchor, const double *sides,
                const int32_t *ncell, int32_t point, const double *view,
                int64_t n, const double *rays, int32_t nf,
                const double *kappa, const double *source, const double *bg,
                int32_t max_cells, double *out) {
  Grid g;
  Camera cam;
  set_grid(&g, anchor, sides, ncell);
  if (!point)
    set_camera(&cam, view[0], view[1]);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  const int64_t width = 3 + (2 + (int64_t)nf) * max_cells + nf;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t k = 0; k < n; ++k) {
    double *o = out + k * width;
    memset(o, 0, sizeof(double) * (size_t)width);
    double *T = malloc(sizeof(double) * (size_t)nf);
    Ray r;
    if (point)
      point_ray(view, rays + 3 * k, &r);
    else
      camera_ray(&cam, rays[2 * k], rays[2 * k + 1], &r);
    double t0, t1;
    int hit;
    const int steps = integrate(
        &g, &r, point, nf, ncells, kappa, source, bg,
        o + 3 + (2 + (int64_t)nf) * max_cells, T, &t0, &t1, &hit, max_cells,
        o + 3, o + 3 + max_cells, o + 3 + 2 * (int64_t)max_cells);
    o[0] = hit ? t0 : NAN;
    o[1] = hit ? t1 : NAN;
    o[2] = (double)steps;
    free(T);
  }
}
