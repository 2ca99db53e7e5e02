/*
 * absorbing_cube_reference.c - CPU restatement of the absorbing line cubes
 * (include/cmi_gpu.h, "absorbing line cubes") in plain C, written from the
 * contract and not from the kernels: the parallel camera's rays and the rays
 * from a point through a box of cells (the geometry of
 * continuum_reference.c), and along them a line whose opacity has the
 * Gaussian profile of its cell, with an optional continuum in the same cell.
 * Every channel of every cell gets the contract's full update; there is no
 * shortcut for cells whose profile misses the band.
 *
 * Built by tests/absorbing_cube_lib.py with gcc -O2 -ffp-contract=off
 * -fopenmp, so that every product and sum below is one IEEE operation, as on
 * the device.
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

/* the clamped error function of the cubes; NaN gives -1 */
static double cube_E(double z) {
  return (z >= 6.) ? 1. : ((z > -6.) ? erf(z) : -1.);
}

/* the cells of a call: a, sl, b and the optional velocity[3][ncells], kc and
 * sc; the velocity axis; frame = the direction to the observer (parallel
 * camera) or the observer's velocity (rays from a point) */
typedef struct {
  const double *a, *sl, *b, *velocity, *kc, *sc, *bg;
  int64_t ncells;
  int32_t nchan;
  double vmin, dv;
  double frame[3];
} Cube;

static void set_cube(Cube *q, const int32_t *ncell, const double *a,
                     const double *sl, const double *b,
                     const double *velocity, const double *kc,
                     const double *sc, const double *bg, int32_t nchan,
                     double vmin, double vmax, const double *frame) {
  q->a = a;
  q->sl = sl;
  q->b = b;
  q->velocity = velocity;
  q->kc = kc;
  q->sc = sc;
  q->bg = bg;
  q->ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  q->nchan = nchan;
  q->vmin = vmin;
  q->dv = (vmax - vmin) / nchan;
  for (int k = 0; k < 3; ++k)
    q->frame[k] = frame ? frame[k] : 0.;
}

/* the radial velocity of a cell as the ray r sees it */
static double radial_velocity(const Cube *q, int64_t cell, const Ray *r,
                              int from_point) {
  double v[3];
  for (int k = 0; k < 3; ++k)
    v[k] = q->velocity ? q->velocity[k * q->ncells + cell] : 0.;
  if (from_point) {
    for (int k = 0; k < 3; ++k)
      v[k] = v[k] - q->frame[k];
    return (v[0] * r->d[0] + v[1] * r->d[1]) + v[2] * r->d[2];
  }
  if (!q->velocity)
    return 0.;
  return -((v[0] * q->frame[0] + v[1] * q->frame[1]) + v[2] * q->frame[2]);
}

/* both integrations of the contract for the nchan channels of one ray; I and
 * T [nchan] are the caller's. Optional trace (max_cells > 0): cells, ds and
 * I[c][i] after step i. Returns the number of crossings. */
static int integrate(const Grid *g, const Cube *q, const Ray *r,
                     int from_point, double *I, double *T, double *t0,
                     double *t1, int *hit_out, int32_t max_cells,
                     double *cells, double *dss, double *I_steps) {
  const int32_t nchan = q->nchan;
  for (int c = 0; c < nchan; ++c) {
    I[c] = from_point ? 0. : (q->bg ? q->bg[c] : 0.);
    T[c] = 1.;
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
      const double adv = q->a[cell] / q->dv;
      const double sl = q->sl[cell], b = q->b[cell];
      const double kc = q->kc ? q->kc[cell] : 0.;
      const double sc = q->sc ? q->sc[cell] : 0.;
      const double u = radial_velocity(q, cell, r, from_point);
      for (int c = 0; c < nchan; ++c) {
        const double e_lo = q->vmin + (double)c * q->dv;
        const double e_hi = q->vmin + (double)(c + 1) * q->dv;
        const double f = 0.5 * (cube_E((e_hi - u) / b) - cube_E((e_lo - u) / b));
        const double al = adv * f;
        const double kappa = al + kc;
        if (kappa != 0.) {
          const double w = al / kappa;
          const double S = sc + w * (sl - sc);
          const double em = expm1(-(kappa * ds));
          if (from_point) {
            I[c] = I[c] + T[c] * (S * -em);
            T[c] = T[c] + T[c] * em;
          } else {
            I[c] = I[c] + em * (I[c] - S);
          }
        }
        if (steps < max_cells)
          I_steps[(int64_t)c * max_cells + steps] = I[c];
      }
      if (steps < max_cells) {
        cells[steps] = (double)cell;
        dss[steps] = ds;
      }
      ++steps;
    }
  }
  if (from_point)
    for (int c = 0; c < nchan; ++c)
      I[c] = I[c] + T[c] * (q->bg ? q->bg[c] : 0.);
  return steps;
}

/* out[c][nx * ny] of the parallel camera; returns the largest number of
 * crossings of a sample ray */
int64_t aref_cube(const double *anchor, const double *sides,
                  const int32_t *ncell, double theta, double phi, int32_t nx,
                  int32_t ny, const double *img_anchor,
                  const double *img_sides, int32_t s, const double *a,
                  const double *sl, const double *b, const double *velocity,
                  const double *kc, const double *sc, const double *bg,
                  int32_t nchan, double vmin, double vmax, double *out) {
  Grid g;
  Camera cam;
  Cube q;
  set_grid(&g, anchor, sides, ncell);
  set_camera(&cam, theta, phi);
  set_cube(&q, ncell, a, sl, b, velocity, kc, sc, bg, nchan, vmin, vmax,
           cam.n);
  const int64_t npixel = (int64_t)nx * ny;
  int64_t longest = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(max : longest)
  for (int64_t pixel = 0; pixel < npixel; ++pixel) {
    const int32_t ix = (int32_t)(pixel / ny), iy = (int32_t)(pixel % ny);
    double *I = malloc(sizeof(double) * 3 * (size_t)nchan);
    double *T = I + nchan, *sum = T + nchan;
    for (int c = 0; c < nchan; ++c)
      sum[c] = 0.;
    for (int sa = 0; sa < s; ++sa)
      for (int sb = 0; sb < s; ++sb) {
        const double fa = (sa + 0.5) / s;
        const double fb = (sb + 0.5) / s;
        const double x = img_anchor[0] + img_sides[0] * ((ix + fa) / nx);
        const double y = img_anchor[1] + img_sides[1] * ((iy + fb) / ny);
        Ray r;
        camera_ray(&cam, x, y, &r);
        double t0, t1;
        const int steps = integrate(&g, &q, &r, 0, I, T, &t0, &t1, NULL, 0,
                                    NULL, NULL, NULL);
        if (steps > longest)
          longest = steps;
        for (int c = 0; c < nchan; ++c)
          sum[c] += I[c];
      }
    for (int c = 0; c < nchan; ++c)
      out[c * npixel + pixel] = sum[c] / (double)(s * s);
    free(I);
  }
  return longest;
}

/* out[c][n] of the rays from origin along directions[n][3]; returns the
 * largest number of crossings of a ray */
int64_t aref_sky_cube(const double *anchor, const double *sides,
                      const int32_t *ncell, const double *origin,
                      const double *v_obs, int64_t n,
                      const double *directions, const double *a,
                      const double *sl, const double *b,
                      const double *velocity, const double *kc,
                      const double *sc, const double *bg, int32_t nchan,
                      double vmin, double vmax, double *out) {
  Grid g;
  Cube q;
  set_grid(&g, anchor, sides, ncell);
  set_cube(&q, ncell, a, sl, b, velocity, kc, sc, bg, nchan, vmin, vmax,
           v_obs);
  int64_t longest = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(max : longest)
  for (int64_t k = 0; k < n; ++k) {
    double *I = malloc(sizeof(double) * 2 * (size_t)nchan);
    double *T = I + nchan;
    Ray r;
    point_ray(origin, directions + 3 * k, &r);
    double t0, t1;
    const int steps = integrate(&g, &q, &r, 1, I, T, &t0, &t1, NULL, 0, NULL,
                                NULL, NULL);
    if (steps > longest)
      longest = steps;
    for (int c = 0; c < nchan; ++c)
      out[c * n + k] = I[c];
    free(I);
  }
  return longest;
}

/* rows {t0, t1, steps, cells[max_cells], ds[max_cells], I[nchan][max_cells],
 * I_end[nchan]}: point == 0, view = {theta, phi}, rays[n][2]; point == 1,
 * view = the origin, rays[n][3] */
void aref_probe(const double *anchor, const double *sides,
                const int32_t *ncell, int32_t point, const double *view,
                const double *v_obs, int64_t n, const double *rays,
                const double *a, const double *sl, const double *b,
                const double *velocity, const double *kc, const double *sc,
                const double *bg, int32_t nchan, double vmin, double vmax,
                int32_t max_cells, double *out) {
  Grid g;
  Camera cam;
  Cube q;
  set_grid(&g, anchor, sides, ncell);
  if (!point)
    set_camera(&cam, view[0], view[1]);
  set_cube(&q, ncell, a, sl, b, velocity, kc, sc, bg, nchan, vmin, vmax,
           point ? v_obs : cam.n);
  const int64_t width = 3 + (2 + (int64_t)nchan) * max_cells + nchan;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t k = 0; k < n; ++k) {
    double *o = out + k * width;
    memset(o, 0, sizeof(double) * (size_t)width);
    double *T = malloc(sizeof(double) * (size_t)nchan);
    Ray r;
    if (point)
      point_ray(view, rays + 3 * k, &r);
    else
      camera_ray(&cam, rays[2 * k], rays[2 * k + 1], &r);
    double t0, t1;
    int hit;
    const int steps = integrate(
        &g, &q, &r, point, o + 3 + (2 + (int64_t)nchan) * max_cells, T, &t0,
        &t1, &hit, max_cells, o + 3, o + 3 + max_cells,
        o + 3 + 2 * (int64_t)max_cells);
    o[0] = hit ? t0 : NAN;
    o[1] = hit ? t1 : NAN;
    o[2] = (double)steps;
    free(T);
  }
}
