/*
 * absorption_reference.c - CPU restatement of the absorption spectra
 * (include/cmi_gpu.h, "absorption spectra") in plain C, written from the
 * contract and not from the kernel: sightlines of finite length through a box
 * of cells (the point camera's clipping and cell walk, as in
 * absorbing_cube_reference.c), and along them the optical depth of K lines
 * with Voigt profiles - the Gaussian core integrated over the channel, the
 * wing term of Tasitsiomi (2006) at its centre - and the column densities.
 * One loop per ray, every channel of every cell with n != 0 gets the full
 * update, no skips.
 *
 * Built by tests/absorption_lib.py with gcc -O2 -ffp-contract=off -fopenmp,
 * so that every product and sum below is one IEEE operation, as on the
 * device; erf is libm's.
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

/* the slab test of a ray that starts at its origin and the first cell; 0 =
 * the ray misses the box */
static int enter(const Grid *g, const Ray *r, double pos[3], int32_t idx[3],
                 double *t0, double *t1) {
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
  const int at_origin = !(tin > 0.);
  *t0 = at_origin ? 0. : tin;
  *t1 = tout;
  if (!hit || !(*t0 < tout) || !(tout < HUGE_VAL))
    return 0;
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

/* one cell crossing: every tying axis advances */
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

/* the wing term Q of H(a, x) = sqrt(pi) Q + exp(-x^2) from x^2 */
static double wing_Q(double a, double x2) {
  const double z = (x2 - 0.855) / (x2 + 3.42);
  double Q = 0.;
  if (z > 0.)
    Q = (1. + 21. / x2) * a / (M_PI * (x2 + 1.)) *
        (z * (0.1117 + z * (4.421 + z * (-9.207 + 5.674 * z))));
  return Q;
}

/* the contract's update of channel c */
static double deposit(double tau, double A, double b, double g, double u,
                      double vmin, double dv, int32_t c) {
  const double e_lo = vmin + (double)c * dv;
  const double e_hi = vmin + (double)(c + 1) * dv;
  const double f = 0.5 * (cube_E((e_hi - u) / b) - cube_E((e_lo - u) / b));
  if (g != 0.) {
    const double x = (0.5 * (e_lo + e_hi) - u) / b;
    const double wing = wing_Q(g / b, x * x) / b;
    return tau + A * (f / dv + wing);
  }
  return tau + A * (f / dv);
}

/* One sightline, K lines: tau[K][nchan] and N[K] are the caller's, zeroed
 * here. Optional trace (max_cells > 0) of line `trace_line`: row = {t0, t1,
 * steps, cells[max_cells], ds[max_cells], tau[ntrace][max_cells],
 * tau_end[ntrace]} for the channels trace_channels. Returns the crossings. */
static int integrate(const Grid *g, const Ray *r, double L, int32_t K,
                     const double *n, const double *b, const double *S,
                     const double *gam, const double *velocity,
                     const double *v_obs, int64_t ncells, int32_t nchan,
                     double vmin, double dv, double *tau, double *N,
                     int32_t ntrace, const int32_t *trace_channels,
                     int32_t max_cells, double *row) {
  double pos[3], t0, t1;
  int32_t idx[3];
  int steps = 0;
  if (tau)
    memset(tau, 0, sizeof(double) * (size_t)K * nchan);
  if (N)
    memset(N, 0, sizeof(double) * (size_t)K);
  double trace_tau[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  const int hit = enter(g, r, pos, idx, &t0, &t1);
  if (hit && L > t0) {
    const double cut = (L < t1) ? L : HUGE_VAL;
    double t = t0;
    int more = 1;
    while (more && inside(g, idx)) {
      const int64_t cell = cell_of(g, idx);
      double ds = step(g, r, pos, idx);
      if (t + ds >= cut) {
        ds = cut - t;
        more = 0;
      }
      t = t + ds;
      double w[3];
      for (int k = 0; k < 3; ++k)
        w[k] = (velocity ? velocity[k * ncells + cell] : 0.) - v_obs[k];
      const double u = (w[0] * r->d[0] + w[1] * r->d[1]) + w[2] * r->d[2];
      for (int32_t l = 0; l < K; ++l) {
        const double nl = n[l * ncells + cell], bl = b[l * ncells + cell];
        if (nl == 0.)
          continue;
        const double nds = nl * ds;
        const double A = nds * S[l];
        if (N)
          N[l] = N[l] + nds;
        if (tau)
          for (int32_t c = 0; c < nchan; ++c)
            tau[l * nchan + c] =
                deposit(tau[l * nchan + c], A, bl, gam[l], u, vmin, dv, c);
        else
          for (int32_t k = 0; k < ntrace; ++k)
            trace_tau[k] = deposit(trace_tau[k], A, bl, gam[l], u, vmin, dv,
                                   trace_channels[k]);
      }
      if (row && steps < max_cells) {
        row[3 + steps] = (double)cell;
        row[3 + max_cells + steps] = ds;
        for (int32_t k = 0; k < ntrace; ++k)
          row[3 + (2 + k) * (int64_t)max_cells + steps] = trace_tau[k];
      }
      ++steps;
    }
  }
  if (row) {
    row[0] = hit ? t0 : NAN;
    row[1] = hit ? t1 : NAN;
    row[2] = (double)steps;
    for (int32_t k = 0; k < ntrace; ++k)
      row[3 + (2 + ntrace) * (int64_t)max_cells + k] = trace_tau[k];
  }
  return steps;
}

static void set_ray(Ray *r, const double *o, const double *d) {
  for (int a = 0; a < 3; ++a) {
    r->o[a] = o[a];
    r->d[a] = d[a];
    r->inv_d[a] = 1. / d[a];
  }
}

/* tau[nrays][K][nchan], N[nrays][K]; returns the largest number of crossings
 * of a ray */
int64_t abref_spectra(const double *anchor, const double *sides,
                      const int32_t *ncell, int32_t K, const double *n,
                      const double *b, const double *S, const double *gam,
                      const double *velocity, int64_t nrays,
                      const double *origins, const double *directions,
                      const double *lengths, const double *observer_velocity,
                      int32_t nchan, double vmin, double vmax, double *tau,
                      double *N) {
  Grid g;
  set_grid(&g, anchor, sides, ncell);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  const double dv = (vmax - vmin) / nchan;
  double v_obs[3];
  for (int k = 0; k < 3; ++k)
    v_obs[k] = observer_velocity ? observer_velocity[k] : 0.;
  int64_t longest = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(max : longest)
  for (int64_t q = 0; q < nrays; ++q) {
    Ray r;
    set_ray(&r, origins + 3 * q, directions + 3 * q);
    const int steps =
        integrate(&g, &r, lengths[q], K, n, b, S, gam, velocity, v_obs,
                  ncells, nchan, vmin, dv, tau + q * (int64_t)K * nchan,
                  N + q * (int64_t)K, 0, NULL, 0, NULL);
    if (steps > longest)
      longest = steps;
  }
  return longest;
}

/* the row of cmi_gpu_absorption_probe */
void abref_probe(const double *anchor, const double *sides,
                 const int32_t *ncell, const double *n, const double *b,
                 double S, double gam, const double *velocity,
                 const double *origin, const double *direction, double length,
                 const double *observer_velocity, int32_t nchan, double vmin,
                 double vmax, int32_t nprobe, const int32_t *channels,
                 int32_t max_cells, double *row) {
  Grid g;
  Ray r;
  set_grid(&g, anchor, sides, ncell);
  set_ray(&r, origin, direction);
  const int64_t ncells = (int64_t)ncell[0] * ncell[1] * ncell[2];
  double v_obs[3];
  for (int k = 0; k < 3; ++k)
    v_obs[k] = observer_velocity ? observer_velocity[k] : 0.;
  integrate(&g, &r, length, 1, n, b, &S, &gam, velocity, v_obs, ncells, nchan,
            vmin, (vmax - vmin) / nchan, NULL, NULL, nprobe, channels,
            max_cells, row);
}
