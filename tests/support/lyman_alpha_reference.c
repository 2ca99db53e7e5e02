/*
 * lyman_alpha_reference.c - CPU restatement of the Lyman-alpha transfer for
 * the tests (include/cmi_gpu.h, "Lyman alpha", has the contract; DESIGN.md
 * 4.17). scattered_cube_reference.c is included below, and with it the
 * restatements it builds on, so that their static functions are the ones
 * used: emit_cell, start, inside, cross, scatter, scatter_towards, cell_of,
 * dot3, dref_pixel. What the mode adds - the records, the Voigt profile, the
 * frequency-dependent marches, the atom's velocity, the Doppler bookkeeping
 * and the delta deposit - is restated here operation for operation, and draws
 * its random numbers in the order the header lists.
 *
 * Built by tests/lyman_alpha_lib.py:
 *   gcc -O2 -ffp-contract=off -fopenmp -shared -fPIC
 *       lyman_alpha_reference.c -L oracle -lcmio
 * The model (grid, dust phase function, camera) is dref_setup's, the source
 * slref_set_field's; lyaref_set builds the records.
 */
#include "scattered_cube_reference.c"

#define LYA_LAMBDA0 1215.67e-10
#define LYA_A21 6.265e8
#define LYA_HYDROGEN_WEIGHT 1.00794
#define LYA_EXP_CUT 64.
#define LYA_MAX_ATTEMPTS 1000000u
#define LYA_ROW 12
#define LYA_HEADER 6

typedef struct {
  double kappa0, inv_b, a, kappa_d, v[3], pad;
} lya_record;

static struct {
  int32_t nchan;
  double vmin, dv, x_crit, x_crit2;
  uint32_t max_scatter;
  lya_record *rec;
  int64_t ncell;
} Y;

/* the records; returns the number of cells that cmi_gpu_set_lyman_alpha
 * would refuse. n_HI may be NULL (then n_H x_H), velocity ([3][ncell]) too */
int64_t lyaref_set(int32_t nchan, double vmin, double vmax, double sigma_turb,
                   double x_crit, uint64_t max_scatter, const double *n_H,
                   const double *x_H, const double *n_HI, const double *T,
                   double sigma_d, const double *velocity) {
  int64_t ncell = 1;
  for (int a = 0; a < 3; ++a)
    ncell *= M.n[a];
  free(Y.rec);
  Y.rec = malloc(sizeof(lya_record) * ncell);
  Y.ncell = ncell;
  Y.nchan = nchan;
  Y.vmin = vmin;
  Y.dv = (vmax - vmin) / nchan;
  Y.x_crit = x_crit;
  Y.x_crit2 = x_crit * x_crit;
  Y.max_scatter = (uint32_t)max_scatter;
  int64_t bad = 0;
  for (int64_t c = 0; c < ncell; ++c) {
    const double nHI = n_HI ? n_HI[c] : n_H[c] * x_H[c];
    const double s2 = SCUBE_BOLTZMANN * T[c] /
                          (LYA_HYDROGEN_WEIGHT * SCUBE_ATOMIC_MASS_UNIT) +
                      sigma_turb * sigma_turb;
    const double b = sqrt(2. * s2);
    if (!(b > 0. && b < HUGE_VAL && nHI >= 0. && nHI < HUGE_VAL &&
          n_H[c] >= 0. && n_H[c] < HUGE_VAL))
      ++bad;
    lya_record *r = Y.rec + c;
    r->kappa0 = nHI *
                (3. * LYA_LAMBDA0 * LYA_LAMBDA0 * LYA_LAMBDA0 * LYA_A21 /
                 (8. * M_PI * sqrt(M_PI))) /
                b;
    r->inv_b = 1. / b;
    r->a = LYA_A21 * LYA_LAMBDA0 / (4. * M_PI * b);
    r->kappa_d = n_H[c] * sigma_d;
    for (int k = 0; k < 3; ++k)
      r->v[k] = velocity ? velocity[k * ncell + c] : 0.;
    r->pad = 0.;
  }
  return bad;
}

/* [ncell][8] */
void lyaref_records(double *out) {
  memcpy(out, Y.rec, sizeof(lya_record) * Y.ncell);
}

static double voigt(double a, double x2) {
  const double z = (x2 - 0.855) / (x2 + 3.42);
  double Q = 0.;
  if (z > 0.)
    Q = (1. + 21. / x2) * a / (M_PI * (x2 + 1.)) *
        (z * (0.1117 + z * (4.421 + z * (-9.207 + 5.674 * z))));
  const double core = (x2 < LYA_EXP_CUT) ? exp(-x2) : 0.;
  return sqrt(M_PI) * Q + core;
}

static double opacity(const lya_record *r, double q, const double k[3],
                      double *kH, double *x) {
  *x = (q - dot3(r->v, k)) * r->inv_b;
  *kH = r->kappa0 * voigt(r->a, *x * *x);
  return *kH + r->kappa_d;
}

/* the depth to the box edge along p->u at the shift q */
static double lya_depth(const photon *p, double q, uint64_t *steps) {
  cursor c;
  start(&c, p->x);
  double tau = 0.;
  int n = 0;
  while (inside(&c)) {
    double op, wall[3], kH, x;
    int64_t cell;
    const double ds = cross(&c, p, &op, wall, &cell);
    tau += ds * opacity(Y.rec + cell, q, p->u, &kH, &x);
    memcpy(c.x, wall, sizeof wall);
    ++n;
  }
  *steps += n;
  return tau;
}

/* interact() with the frequency-dependent opacity */
static int lya_interact(photon *p, double q, double tau, uint64_t *steps) {
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
    if (tau < 0.) {
      const double back = ds * tau / dtau;
      for (int a = 0; a < 3; ++a)
        c.x[a] += (wall[a] - c.x[a]) * (ds + back) / ds;
      memcpy(c.i, before, sizeof before);
    } else {
      memcpy(c.x, wall, sizeof wall);
    }
    ++n;
  }
  *steps += n;
  memcpy(p->x, c.x, sizeof c.x);
  return n > 0 && inside(&c);
}

static double separation(double x, double a) {
  const double la = log10(a);
  const double x_cw = 1.59 - 0.60 * la - 0.03 * la * la;
  if (x < 0.2)
    return 0.;
  if (x < x_cw)
    return fmax(0., x - 0.01 * pow(a, 1. / 6.) * exp(1.2 * x));
  return fmin(4., fmax(0., x - 0.5));
}

/* *margin (if not NULL) receives the smallest relative distance of a
 * decision of this draw from its threshold */
static double sample_parallel(double x, double a, stream *s, uint64_t *nrej,
                              double *margin) {
  const double ax = fabs(x);
  const double u0 = separation(ax, a);
  const double e0 = exp(-(u0 * u0));
  const double th0 = atan((u0 - ax) / a);
  const double p = (th0 + M_PI_2) / ((1. - e0) * th0 + (1. + e0) * M_PI_2);
  double u = 0.;
  for (uint32_t attempt = 0; attempt < LYA_MAX_ATTEMPTS; ++attempt) {
    const double R1 = uniform(s);
    const double R2 = uniform(s);
    const double R3 = uniform(s);
    int accept;
    double bound;
    if (R1 <= p) {
      const double th = -M_PI_2 + R2 * (th0 + M_PI_2);
      u = a * tan(th) + ax;
      bound = exp(-(u * u));
    } else {
      const double th = th0 + R2 * (M_PI_2 - th0);
      u = a * tan(th) + ax;
      bound = exp(-(u * u)) / e0;
    }
    accept = R3 <= bound;
    if (margin) {
      const double m1 = fabs(R1 - p) / p;
      const double m3 = fabs(R3 - bound) / R3;
      if (m1 < *margin)
        *margin = m1;
      if (m3 < *margin)
        *margin = m3;
    }
    if (accept)
      break;
    ++*nrej;
  }
  return (x < 0.) ? -u : u;
}

static void isotropic(stream *s, photon *p) {
  const double mu = 2. * uniform(s) - 1.;
  const double smu = sqrt(fmax(1. - mu * mu, 0.));
  const double az = 2. * M_PI * uniform(s);
  p->ang[0] = smu;
  p->ang[1] = mu;
  p->ang[2] = az;
  p->ang[3] = sin(az);
  p->ang[4] = cos(az);
  point(p, smu * p->ang[4], smu * p->ang[3], mu);
}

static int32_t channel_of(double u) {
  const double f = floor((u - Y.vmin) / Y.dv);
  if (!(f >= -1.) || !(f <= (double)Y.nchan))
    return -1;
  int32_t c = (int32_t)f;
  if (u < Y.vmin + (double)c * Y.dv)
    --c;
  else if (u >= Y.vmin + (double)(c + 1) * Y.dv)
    ++c;
  return (c >= 0 && c < Y.nchan) ? c : -1;
}

typedef struct {
  double *image;   /* [npixel] or NULL */
  double *cube;    /* [nchan][npixel] */
  double *squares; /* [2][nchan][npixel] or NULL */
  double *rows;    /* trace rows or NULL */
  int max_rows, nrows;
  int64_t npixel;
  uint64_t steps, hydrogen, dust, rejections, atomics, capped, packets;
  double margin; /* smallest relative distance of a decision from its
                    threshold */
} lya_sink;

static void lya_peel(lya_sink *y, const photon *p, int species, double q,
                     const double w[3], double W, double u_par, double x) {
  photon peel = *p;
  const double wd = dot3(w, M.obs);
  double factor, q_d;
  if (species == 2) {
    factor = scatter_towards(&peel);
    q_d = q + (wd - dot3(w, p->u));
  } else {
    factor = 0.25 / M_PI;
    q_d = (species == 0) ? wd : q + (wd - dot3(w, p->u));
  }
  photon view = *p;
  point(&view, M.obs[0], M.obs[1], M.obs[2]);
  const double tau = lya_depth(&view, q_d, &y->steps);
  const double addend = ((W * factor) * exp(-tau)) * peel.iquv[0];
  const double u = -q_d;
  if (y->rows) {
    if (y->nrows < y->max_rows) {
      double *r = y->rows + LYA_ROW * y->nrows;
      memcpy(r, p->x, 3 * sizeof(double));
      memcpy(r + 3, p->u, 3 * sizeof(double));
      r[6] = q;
      r[7] = addend;
      r[8] = (double)species;
      r[9] = u;
      r[10] = u_par;
      r[11] = x;
    }
    ++y->nrows;
  }
  if (!y->image)
    return;
  const int64_t px = dref_pixel(p->x);
  if (px < 0 || addend == 0.)
    return;
  y->image[px] += addend;
  ++y->atomics;
  const int32_t ch = channel_of(u);
  if (ch >= 0) {
    y->cube[ch * y->npixel + px] += addend;
    ++y->atomics;
    if (y->squares) {
      y->squares[ch * y->npixel + px] += addend * addend;
      y->squares[(Y.nchan + ch) * y->npixel + px] += 1.;
    }
  }
}

static void lya_packet(uint32_t seed, uint64_t id, lya_sink *y) {
  stream s = {seed, id, 0u};
  photon p;
  ++y->packets;
  const int64_t ecell = emit_cell(&s, &p);
  {
    const lya_record *r = Y.rec + ecell;
    const double b = 1. / r->inv_b;
    const double r1 = sqrt(-log(uniform(&s)));
    const double f1 = 2. * M_PI * uniform(&s);
    const double r2 = sqrt(-log(uniform(&s)));
    const double f2 = 2. * M_PI * uniform(&s);
    const double w[3] = {r->v[0] + b * (r1 * cos(f1)),
                         r->v[1] + b * (r1 * sin(f1)),
                         r->v[2] + b * (r2 * cos(f2))};
    const double q0 = dot3(w, p.u);
    lya_peel(y, &p, 0, q0, w, 1., 0., 0.);
    double q = q0;
    const double forced = 1. - exp(-lya_depth(&p, q, &y->steps));
    double albedo = 1.;
    int alive =
        lya_interact(&p, q, -log(1. - uniform(&s) * forced), &y->steps);
    uint32_t n = 0;
    while (alive) {
      const lya_record *c = Y.rec + cell_of(p.x);
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
      alive = lya_interact(&p, q, -log(uniform(&s)), &y->steps);
    }
  }
}

/* ------------------------------------------------------------ probes -- */
void lyaref_voigt(int64_t n, const double *in, double *out) {
  for (int64_t k = 0; k < n; ++k) {
    const double *r = in + 4 * k;
    out[2 * k] = voigt(r[0], r[1] * r[1]);
    out[2 * k + 1] = r[2] * out[2 * k] + r[3];
  }
}

void lyaref_optical_depth(int64_t n, const double *in, double *out) {
  for (int64_t k = 0; k < n; ++k) {
    photon p;
    memcpy(p.x, in + 7 * k, 3 * sizeof(double));
    point(&p, in[7 * k + 3], in[7 * k + 4], in[7 * k + 5]);
    uint64_t steps = 0;
    out[2 * k] = lya_depth(&p, in[7 * k + 6], &steps);
    out[2 * k + 1] = (double)steps;
  }
}

/* out {u_par, rejections}; margins[n] (may be NULL) the smallest relative
 * distance of a decision from its threshold */
void lyaref_sampler(uint32_t seed, uint64_t first, int64_t n, const double *in,
                    double *out, double *margins) {
#pragma omp parallel for schedule(static)
  for (int64_t k = 0; k < n; ++k) {
    stream s = {seed, first + k, 0u};
    uint64_t nrej = 0;
    double margin = HUGE_VAL;
    out[2 * k] = sample_parallel(in[2 * k], in[2 * k + 1], &s, &nrej, &margin);
    out[2 * k + 1] = (double)nrej;
    if (margins)
      margins[k] = margin;
  }
}

/* rows {events, hydrogen, dust, steps, capped, rejections, rows[max_events]
 * [12]}; margins[n] as above */
void lyaref_trace(uint32_t seed, uint64_t first, int64_t n, double *out,
                  int32_t max_events, double *margins) {
  const int w = LYA_HEADER + LYA_ROW * max_events;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t k = 0; k < n; ++k) {
    lya_sink y;
    memset(&y, 0, sizeof y);
    y.rows = out + w * k + LYA_HEADER;
    y.max_rows = max_events;
    y.margin = HUGE_VAL;
    lya_packet(seed, first + k, &y);
    out[w * k] = y.nrows;
    out[w * k + 1] = (double)y.hydrogen;
    out[w * k + 2] = (double)y.dust;
    out[w * k + 3] = (double)y.steps;
    out[w * k + 4] = (double)y.capped;
    out[w * k + 5] = (double)y.rejections;
    if (margins)
      margins[k] = y.margin;
  }
}

/* the whole run: image [npixel], cube [nchan][npixel], squares [2][nchan]
 * [npixel] (may be NULL), all added to; counters {steps, hydrogen, dust,
 * rejections, deposits, capped, packets}; *margin (may be NULL) the smallest
 * relative distance of any decision of the run from its threshold */
void lyaref_shoot(uint32_t seed, uint64_t first, int64_t n, double *image,
                  double *cube, double *squares, uint64_t counters[7],
                  double *margin) {
  const int64_t np = (int64_t)M.res[0] * M.res[1];
  const int64_t nc = Y.nchan * np, ns = 2 * nc;
  uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
  double least = HUGE_VAL;
#pragma omp parallel reduction(+ : c0, c1, c2, c3, c4, c5, c6) reduction(min : least)
  {
    double *mine = calloc(np + nc + ns, sizeof(double));
    lya_sink y;
    memset(&y, 0, sizeof y);
    y.image = mine;
    y.cube = mine + np;
    y.squares = squares ? mine + np + nc : 0;
    y.npixel = np;
    y.margin = HUGE_VAL;
#pragma omp for schedule(dynamic, 16)
    for (int64_t k = 0; k < n; ++k)
      lya_packet(seed, first + k, &y);
#pragma omp critical
    {
      for (int64_t i = 0; i < np; ++i)
        image[i] += mine[i];
      for (int64_t i = 0; i < nc; ++i)
        cube[i] += mine[np + i];
      if (squares)
        for (int64_t i = 0; i < ns; ++i)
          squares[i] += mine[np + nc + i];
    }
    free(mine);
    c0 += y.steps;
    c1 += y.hydrogen;
    c2 += y.dust;
    c3 += y.rejections;
    c4 += y.atomics;
    c5 += y.capped;
    c6 += y.packets;
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
  if (margin)
    *margin = least;
}
