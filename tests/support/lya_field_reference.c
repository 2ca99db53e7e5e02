/*
 * lya_field_reference.c - CPU restatement of the Lyman-alpha radiation field
 * for the tests (include/cmi_gpu.h, "Lyman alpha radiation field", has the
 * contract). lyman_alpha_reference.c is included below, and
 * with it the restatements it builds on, so that their static functions are
 * the ones used: the records, opacity, the atom sampler, the peel-off and the
 * cursor of the march. What the field adds is restated here: the two marches
 * with their tallies, the packet's life with the collision estimators (a copy
 * of lya_packet, event for event and draw for draw), and the coupling formula.
 *
 * Built by tests/lya_field_lib.py:
 *   gcc -O2 -ffp-contract=off -fopenmp -shared -fPIC
 *       lya_field_reference.c -L oracle -lcmio
 */
#include "lyman_alpha_reference.c"

#define LYAF_ROW 8
enum { F_L = 0, F_SH = 1, F_SD = 2, F_G = 3, F_NH = 6, F_ND = 7 };

#define LYAF_PLANCK 6.626070040e-34
#define LYAF_LIGHTSPEED 299792458.
#define LYAF_HI_FREQUENCY 1420405751.768
#define LYAF_HI_EINSTEIN_A 2.8843e-15

/* what a packet adds beyond the sink of the images */
typedef struct {
  double *rows;      /* [ncell][8] */
  double *crossings; /* [ncell]: tallied crossings per cell, or NULL */
  double chord;      /* length of the first flights */
  double momentum[3]; /* sum of forced * (k_first - k_last) */
  uint64_t walk_steps; /* tallied crossings */
  uint64_t march_steps; /* crossings of the packets' own marches: all but
                           the peel-off's */
} field_sink;

static double mean_transmission(double t) {
  return (t > 0.) ? -expm1(-t) / t : 1.;
}

static void tally_flight(field_sink *f, int64_t cell, double len, double kH,
                         double kd, const double k[3]) {
  double *row = f->rows + LYAF_ROW * cell;
  const double push = len * (kH + kd * (1. - M.albedo * M.g));
  row[F_L] += len;
  row[F_SH] += len * kH;
  row[F_SD] += len * kd;
  for (int a = 0; a < 3; ++a)
    row[F_G + a] += push * k[a];
  if (f->crossings)
    f->crossings[cell] += 1.;
  ++f->walk_steps;
}

/* lya_depth() of the first flight: the expected value */
static double field_depth(const photon *p, double q, uint64_t *steps,
                          field_sink *f) {
  cursor c;
  start(&c, p->x);
  double tau = 0.;
  int n = 0;
  while (inside(&c)) {
    double op, wall[3], kH, x;
    int64_t cell;
    const double ds = cross(&c, p, &op, wall, &cell);
    const double dtau = ds * opacity(Y.rec + cell, q, p->u, &kH, &x);
    tally_flight(f, cell, 1. * ((ds * exp(-tau)) * mean_transmission(dtau)),
                 kH, Y.rec[cell].kappa_d, p->u);
    f->chord += ds;
    tau += dtau;
    memcpy(c.x, wall, sizeof wall);
    ++n;
  }
  *steps += n;
  return tau;
}

/* lya_interact() with the track-length tally of weight W */
static int field_interact(photon *p, double q, double tau, uint64_t *steps,
                          field_sink *f, double W) {
  cursor c;
  start(&c, p->x);
  int n = 0;
  while (inside(&c) && tau > 0.) {
    const int32_t before[3] = {c.i[0], c.i[1], c.i[2]};
    double op, wall[3], kH, x;
    int64_t cell;
    const double ds = cross(&c, p, &op, wall, &cell);
    const double dtau = ds * opacity(Y.rec + cell, q, p->u, &kH, &x);
    tau -= dtau;
    double flown = ds;
    if (tau < 0.) {
      const double back = ds * tau / dtau;
      flown = ds + back;
      for (int a = 0; a < 3; ++a)
        c.x[a] += (wall[a] - c.x[a]) * (ds + back) / ds;
      memcpy(c.i, before, sizeof before);
    } else {
      memcpy(c.x, wall, sizeof wall);
    }
    tally_flight(f, cell, W * flown, kH, Y.rec[cell].kappa_d, p->u);
    ++n;
  }
  *steps += n;
  memcpy(p->x, c.x, sizeof c.x);
  return n > 0 && inside(&c);
}

/* lya_packet() with the field */
static void field_packet(uint32_t seed, uint64_t id, lya_sink *y,
                         field_sink *f) {
  stream s = {seed, id, 0u};
  photon p;
  ++y->packets;
  const int64_t ecell = emit_cell(&s, &p);
  const lya_record *r = Y.rec + ecell;
  const double b = 1. / r->inv_b;
  const double r1 = sqrt(-log(uniform(&s)));
  const double f1 = 2. * M_PI * uniform(&s);
  const double r2 = sqrt(-log(uniform(&s)));
  const double f2 = 2. * M_PI * uniform(&s);
  const double w[3] = {r->v[0] + b * (r1 * cos(f1)),
                       r->v[1] + b * (r1 * sin(f1)),
                       r->v[2] + b * (r2 * cos(f2))};
  const double k_first[3] = {p.u[0], p.u[1], p.u[2]};
  uint64_t march = 0;
  double q = dot3(w, p.u);
  lya_peel(y, &p, 0, q, w, 1., 0., 0.);
  const double forced = 1. - exp(-field_depth(&p, q, &march, f));
  double albedo = 1.;
  int alive = lya_interact(&p, q, -log(1. - uniform(&s) * forced), &march);
  uint32_t n = 0;
  while (alive) {
    const int64_t cell = cell_of(p.x);
    const lya_record *c = Y.rec + cell;
    const double k[3] = {p.u[0], p.u[1], p.u[2]};
    double kH, x;
    const double kappa = opacity(c, q, k, &kH, &x);
    const double R = uniform(&s);
    const double PH = kH / kappa;
    if (PH < 1.) {
      const double m = fabs(R - PH) / R;
      if (m < y->margin)
        y->margin = m;
    }
    if (R < PH) {
      f->rows[LYAF_ROW * cell + F_NH] += forced * albedo;
      const double bc = 1. / c->inv_b;
      const double u_par =
          sample_parallel(x, c->a, &s, &y->rejections, &y->margin);
      const double skip = (fabs(x) < Y.x_crit) ? Y.x_crit2 : 0.;
      const double rho = sqrt(skip - log(uniform(&s)));
      const double psi = 2. * M_PI * uniform(&s);
      const double u1 = rho * cos(psi), u2 = rho * sin(psi);
      const double e1[3] = {p.ang[1] * p.ang[4], p.ang[1] * p.ang[3],
                            -p.ang[0]};
      const double e2[3] = {-p.ang[3], p.ang[4], 0.};
      double wa[3];
      for (int a = 0; a < 3; ++a)
        wa[a] = c->v[a] + bc * ((u_par * k[a] + u1 * e1[a]) + u2 * e2[a]);
      lya_peel(y, &p, 1, q, wa, forced * albedo, u_par, x);
      isotropic(&s, &p);
      p.iquv[1] = p.iquv[2] = p.iquv[3] = 0.;
      q += dot3(wa, p.u) - dot3(wa, k);
      ++y->hydrogen;
    } else {
      f->rows[LYAF_ROW * cell + F_ND] += forced * albedo;
      albedo *= M.albedo;
      lya_peel(y, &p, 2, q, c->v, forced * albedo, 0., x);
      scatter(&s, &p);
      q += dot3(c->v, p.u) - dot3(c->v, k);
      ++y->dust;
    }
    if (++n >= Y.max_scatter) {
      ++y->capped;
      break;
    }
    alive = field_interact(&p, q, -log(uniform(&s)), &march, f,
                           forced * albedo);
  }
  y->steps += march;
  f->march_steps += march;
  for (int a = 0; a < 3; ++a)
    f->momentum[a] += forced * (k_first[a] - p.u[a]);
}

/* the whole run with the field: lyaref_shoot's image [npixel], cube [nchan]
 * [npixel] and counters[7], and rows [ncell][8], crossings [ncell] (may be
 * NULL), all added to; sums {chord length of the first flights, momentum[3] =
 * sum of forced (k_first - k_last), tallied crossings, crossings of all
 * marches but the peel-off's}; *margin as there */
void lyafref_shoot(uint32_t seed, uint64_t first, int64_t n, double *image,
                   double *cube, uint64_t counters[7], double *rows,
                   double *crossings, double sums[6], double *margin) {
  const int64_t np = (int64_t)M.res[0] * M.res[1];
  const int64_t nc = Y.nchan * np, nr = LYAF_ROW * Y.ncell;
  const int64_t nx = crossings ? Y.ncell : 0;
  uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, ws = 0, ms = 0;
  double least = HUGE_VAL, chord = 0., m0 = 0., m1 = 0., m2 = 0.;
#pragma omp parallel reduction(+ : c0, c1, c2, c3, c4, c5, c6, ws, ms, chord, m0, m1, m2) reduction(min : least)
  {
    double *mine = calloc(np + nc + nr + nx, sizeof(double));
    lya_sink y;
    field_sink f;
    memset(&y, 0, sizeof y);
    memset(&f, 0, sizeof f);
    y.image = mine;
    y.cube = mine + np;
    y.npixel = np;
    y.margin = HUGE_VAL;
    f.rows = mine + np + nc;
    f.crossings = crossings ? mine + np + nc + nr : 0;
#pragma omp for schedule(dynamic, 16)
    for (int64_t k = 0; k < n; ++k)
      field_packet(seed, first + k, &y, &f);
#pragma omp critical
    {
      for (int64_t i = 0; i < np; ++i)
        image[i] += mine[i];
      for (int64_t i = 0; i < nc; ++i)
        cube[i] += mine[np + i];
      for (int64_t i = 0; i < nr; ++i)
        rows[i] += mine[np + nc + i];
      for (int64_t i = 0; i < nx; ++i)
        crossings[i] += mine[np + nc + nr + i];
    }
    free(mine);
    c0 += y.steps;
    c1 += y.hydrogen;
    c2 += y.dust;
    c3 += y.rejections;
    c4 += y.atomics;
    c5 += y.capped;
    c6 += y.packets;
    ws += f.walk_steps;
    ms += f.march_steps;
    chord += f.chord;
    m0 += f.momentum[0];
    m1 += f.momentum[1];
    m2 += f.momentum[2];
    if (y.margin < least)
      least = y.margin;
  }
  counters[0] = c0;
  counters[1] = c1;
  counters[2] = c2;
  counters[3] = c3;
  counters[4] = c4;
  counters[5] = c5;
  counters[6] = c6;
  sums[0] = chord;
  sums[1] = m0;
  sums[2] = m1;
  sums[3] = m2;
  sums[4] = (double)ws;
  sums[5] = (double)ms;
  if (margin)
    *margin = least;
}

/* ---------------------------------------------------------- coupling -- */

/* P_alpha = s S_H / (h nu_0 n_HI V), 0 where n_HI = 0 */
void lyafref_scattering_rate(int64_t n, const double *rows, const double *n_HI,
                             double scale, double volume, double *P) {
  for (int64_t c = 0; c < n; ++c)
    P[c] = (n_HI[c] > 0.)
               ? scale * rows[LYAF_ROW * c + F_SH] /
                     ((LYAF_PLANCK * LYAF_LIGHTSPEED / LYA_LAMBDA0) * n_HI[c] *
                      volume)
               : 0.;
}

static double kappa_HH(double T) {
  return 3.1e-17 * pow(T, 0.357) * exp(-32. / T);
}

static double kappa_eH(double T) {
  const double lT = log10(fmin(fmax(T, 1.), 1.e4));
  return 1.e-6 * pow(10., -9.607 + 0.5 * lT * exp(-pow(lT, 4.5) / 1800.));
}

/* T_s of n cells from {T, n_HI, n_e, P_alpha} */
void lyafref_spin_temperature(int64_t n, const double *T, const double *n_HI,
                              const double *n_e, const double *P,
                              double T_gamma, int32_t collisions,
                              double *T_s) {
  const double T_star = LYAF_PLANCK * LYAF_HI_FREQUENCY / SCUBE_BOLTZMANN;
  for (int64_t c = 0; c < n; ++c) {
    if (!(T[c] > 0.)) {
      T_s[c] = T_gamma;
      continue;
    }
    const double C_10 =
        collisions ? n_HI[c] * kappa_HH(T[c]) + n_e[c] * kappa_eH(T[c]) : 0.;
    const double x_a = 4. * P[c] * T_star / (27. * LYAF_HI_EINSTEIN_A * T_gamma);
    const double x_c = (C_10 / LYAF_HI_EINSTEIN_A) * (T_star / T_gamma);
    const double x = x_a + x_c;
    T_s[c] = (1. + x) / (1. / T_gamma + x / T[c]);
  }
}
