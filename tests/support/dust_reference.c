/*
 * dust_reference.c - CPU restatement of the dusty radiative transfer mode
 * (DustSimulation, src/DustSimulation.cpp:67-186) for the tests: the device
 * path (cmacionize_amd/csrc/device_dust.h, dust_kernels.h) is checked
 * against it on the same random streams.
 *
 * Built by the test that uses it:
 *   gcc -O2 -ffp-contract=off -fopenmp -shared -fPIC dust_reference.c
 *       -L oracle -lcmio
 * It takes the packet random numbers (cmio_rng_uniform) and the cell wall
 * intersection (cmio_wall_intersection) from the oracle library and draws
 * in the order device_dust.h documents. One model at a time (dref_setup).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif
#define INV_PI M_1_PI

double cmio_rng_uniform(uint32_t seed, uint32_t iteration, uint64_t packet,
                        uint32_t draw);
void cmio_wall_intersection(const double origin[3], const double direction[3],
                            const double inverse_direction[3],
                            const double cell_anchor[3],
                            const double cell_sides[3], int32_t next_index[3],
                            double *ds, double intersection[3]);

#define DREF_MAX_SCATTER 100000
#define DREF_MAX_ATTEMPTS 1000000u /* the source's rejection loop */

/* ------------------------------------------------------------- model -- */
static struct {
  /* CartesianDensityGrid (src/CartesianDensityGrid.cpp:40-95) */
  double anchor[3], sides[3], cell[3], inv_cell[3];
  int32_t n[3];
  double *opacity; /* n kappa x_H per cell */
  /* DustScattering (src/DustScattering.hpp:171-185) */
  double g, one_minus_g2, two_g, one_minus_g, half_over_g, one_plus_g2, pl,
      albedo;
  /* CCDImage (src/CCDImage.hpp:123-160) */
  double st, ct, ph, sp, cp; /* observer angles */
  double obs[3];
  int32_t res[2];
  double ia[2], is[2];
  /* SpiralGalaxyContinuousPhotonSource
   * (src/SpiralGalaxyContinuousPhotonSource.hpp:98-150) */
  double r_c, r_b, r_j, rs, hs, bt, qb, qc;
  double cdf_w[1001], cdf_p[1001];
} M;

typedef struct {
  uint32_t seed;
  uint64_t id;
  uint32_t next;
} stream;

static double uniform(stream *s) {
  return cmio_rng_uniform(s->seed, 0u, s->id, s->next++);
}

typedef struct {
  double x[3], u[3], iu[3];
  double ang[5]; /* sin theta, cos theta, phi, sin phi, cos phi */
  double iquv[4];
} photon;

static void point(photon *p, double ux, double uy, double uz) {
  p->u[0] = ux;
  p->u[1] = uy;
  p->u[2] = uz;
  for (int a = 0; a < 3; ++a)
    p->iu[a] = 1. / p->u[a];
}

int dref_setup(const double anchor[3], const double sides[3],
               const int32_t ncell[3], const double *number_density,
               const double *x_H, double g, double p_l, double albedo,
               double kappa, double theta, double phi, int32_t nx, int32_t ny,
               const double img_anchor[2], const double img_sides[2],
               double r_stars, double h_stars, double bulge_over_total) {
  int64_t ntot = 1;
  for (int a = 0; a < 3; ++a) {
    M.anchor[a] = anchor[a];
    M.sides[a] = sides[a];
    M.n[a] = ncell[a];
    M.cell[a] = sides[a] / ncell[a];
    M.inv_cell[a] = 1. / M.cell[a];
    ntot *= ncell[a];
  }
  free(M.opacity);
  M.opacity = malloc(sizeof(double) * ntot);
  if (!M.opacity)
    return 1;
  for (int64_t i = 0; i < ntot; ++i)
    M.opacity[i] = number_density[i] * kappa * x_H[i];
  M.g = g;
  M.one_minus_g2 = 1. - g * g;
  M.two_g = 2. * g;
  M.one_minus_g = 1. - g;
  M.half_over_g = 0.5 / g;
  M.one_plus_g2 = 1. + g * g;
  M.pl = p_l;
  M.albedo = albedo;
  M.st = sin(theta);
  M.ct = cos(theta);
  M.ph = phi;
  M.sp = sin(phi);
  M.cp = cos(phi);
  M.obs[0] = M.st * M.cp;
  M.obs[1] = M.st * M.sp;
  M.obs[2] = M.ct;
  M.res[0] = nx;
  M.res[1] = ny;
  M.ia[0] = img_anchor[0];
  M.ia[1] = img_anchor[1];
  M.is[0] = img_sides[0];
  M.is[1] = img_sides[1];
  const double kpc = 3.086e19;
  M.r_c = 0.2 * kpc;
  M.r_b = 2. * kpc;
  M.r_j = 0.4 * kpc;
  M.rs = r_stars;
  M.hs = h_stars;
  M.qb = M.r_b / (M.r_b + M.r_j);
  M.qc = M.r_c / (M.r_c + M.r_j);
  M.bt = bulge_over_total * (1. - M.qc / M.qb);
  const double wmax = 1.2 * sqrt(anchor[0] * anchor[0] +
                                 anchor[1] * anchor[1] + anchor[2] * anchor[2]);
  for (int i = 0; i < 1000; ++i) {
    const double w = i * wmax / 1000;
    M.cdf_w[i] = w;
    M.cdf_p[i] = 1. - (1. + w / r_stars) * exp(-(w / r_stars));
  }
  M.cdf_w[1000] = wmax;
  M.cdf_p[1000] = 1.;
  return 0;
}

/* the disc CDF as built, for the tests */
void dref_disc_cdf(double *w, double *p) {
  memcpy(w, M.cdf_w, sizeof M.cdf_w);
  memcpy(p, M.cdf_p, sizeof M.cdf_p);
}

/* ------------------------------------------------------------ source -- */
static int in_box(const double x[3]) {
  for (int a = 0; a < 3; ++a)
    if (!(x[a] >= M.anchor[a] && x[a] < M.anchor[a] + M.sides[a]))
      return 0;
  return 1;
}

/* Utilities::locate (src/Utilities.hpp:726-742): bisection for the last
 * entry below x, never the last index */
static int bracket(double x) {
  int lo = 0, hi = 1001;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (x > M.cdf_p[mid])
      lo = mid;
    else
      hi = mid;
  }
  return lo == 1000 ? 999 : lo;
}

/* src/SpiralGalaxyContinuousPhotonSource.hpp:277-334, then
 * src/DustPhotonShootJob.hpp:113-125 */
static int emit(stream *s, photon *p) {
  (void)uniform(s); /* PhotonSource::get_random_photon's selector */
  for (int a = 0; a < 3; ++a)
    p->x[a] = M.anchor[a] - M.sides[a];
  for (uint32_t tries = 0; !in_box(p->x); ++tries) {
    if (tries == DREF_MAX_ATTEMPTS)
      return 0; /* no position: dropped */
    if (uniform(s) <= M.bt) {
      const double u = uniform(s);
      const double A = u * M.qb + (1. - u) * M.qc;
      const double r = M.r_j / (1. / A - 1.);
      const double az = 2. * M_PI * uniform(s);
      const double mu = 2. * uniform(s) - 1.;
      const double smu = sqrt(fmax(1. - mu * mu, 0.));
      p->x[0] = r * smu * cos(az);
      p->x[1] = r * smu * sin(az);
      p->x[2] = r * mu;
    } else {
      const double v = 2. * uniform(s) - 1.;
      const double z = v > 0. ? -M.hs * log(v) : M.hs * log(-v);
      const double az = 2. * M_PI * uniform(s);
      const double q = uniform(s);
      const int i = bracket(q);
      const double w = M.cdf_w[i] + (q - M.cdf_p[i]) /
                                        (M.cdf_p[i + 1] - M.cdf_p[i]) *
                                        (M.cdf_w[i + 1] - M.cdf_w[i]);
      p->x[0] = w * cos(az);
      p->x[1] = w * sin(az);
      p->x[2] = z;
    }
  }
  (void)uniform(s); /* the source's own direction, discarded */
  (void)uniform(s);
  const double mu = 2. * uniform(s) - 1.;
  const double smu = sqrt(fmax(1. - mu * mu, 0.));
  const double az = 2. * M_PI * uniform(s);
  p->ang[0] = smu;
  p->ang[1] = mu;
  p->ang[2] = az;
  p->ang[3] = sin(az);
  p->ang[4] = cos(az);
  point(p, smu * p->ang[4], smu * p->ang[3], mu);
  p->iquv[0] = 1.;
  p->iquv[1] = p->iquv[2] = p->iquv[3] = 0.;
  return 1;
}

/* ------------------------------------------------------------- march -- */
typedef struct {
  double x[3];
  int32_t i[3];
} cursor;

/* CartesianDensityGrid::get_cell_indices (src/CartesianDensityGrid.cpp:
 * 152-161) */
static void start(cursor *c, const double x[3]) {
  for (int a = 0; a < 3; ++a) {
    c->x[a] = x[a];
    c->i[a] = (int32_t)((x[a] - M.anchor[a]) * M.inv_cell[a]);
  }
}

static int inside(const cursor *c) {
  for (int a = 0; a < 3; ++a)
    if (c->i[a] < 0 || c->i[a] >= M.n[a])
      return 0;
  return 1;
}

/* one cell: path length to the next wall (cmio_wall_intersection), the
 * cell's opacity; moves the cursor to the wall */
static double cross(cursor *c, const photon *p, double *op, double wall[3],
                    int64_t *cell) {
  double lo[3];
  int32_t step[3];
  double ds;
  for (int a = 0; a < 3; ++a)
    lo[a] = M.anchor[a] + M.cell[a] * c->i[a];
  cmio_wall_intersection(c->x, p->u, p->iu, lo, M.cell, step, &ds, wall);
  *cell = ((int64_t)c->i[0] * M.n[1] + c->i[1]) * M.n[2] + c->i[2];
  *op = M.opacity[*cell];
  for (int a = 0; a < 3; ++a)
    c->i[a] += step[a];
  return ds;
}

/* src/CartesianDensityGrid.cpp:328-363 */
static double optical_depth(const photon *p, uint64_t *steps, double *cells,
                            int max_cells) {
  cursor c;
  start(&c, p->x);
  double tau = 0.;
  int k = 0;
  while (inside(&c)) {
    double op, wall[3];
    int64_t cell;
    const double ds = cross(&c, p, &op, wall, &cell);
    tau += ds * op;
    memcpy(c.x, wall, sizeof wall);
    if (cells && k < max_cells)
      cells[k] = (double)cell;
    ++k;
  }
  *steps += k;
  return tau;
}

/* src/CartesianDensityGrid.cpp:375-452; 0 = the photon left (end()) */
static int interact(photon *p, double tau, uint64_t *steps) {
  cursor c;
  start(&c, p->x);
  int k = 0;
  while (inside(&c) && tau > 0.) {
    const int32_t before[3] = {c.i[0], c.i[1], c.i[2]};
    double op, wall[3];
    int64_t cell;
    const double ds = cross(&c, p, &op, wall, &cell);
    const double dtau = ds * op;
    tau -= dtau;
    if (tau < 0.) {
      /* stops inside the cell: back off along the segment */
      const double corr = ds * tau / dtau;
      for (int a = 0; a < 3; ++a)
        c.x[a] += (wall[a] - c.x[a]) * (ds + corr) / ds;
      memcpy(c.i, before, sizeof before);
    } else {
      memcpy(c.x, wall, sizeof wall);
    }
    ++k;
  }
  *steps += k;
  memcpy(p->x, c.x, sizeof c.x);
  return k > 0 && inside(&c);
}

/* -------------------------------------------------------- scattering -- */

/* Code & Whitney (1995) eq. 2 with White (1979) eqs. 3-6: the Mueller
 * product for a rotation into / out of the scattering plane by angles with
 * cosines and sines of twice them (c1, s1) and (c2, s2). `mirror` selects
 * the half of the azimuth above pi, where the reference flips signs
 * (src/DustScattering.cpp:177-229 vs :231-282, :391-441 vs :443-491). */
static void mueller(double P1, double P2, double P3, double P4, double c1,
                    double s1, double c2, double s2, int mirror,
                    const double in[4], double out[4]) {
  const double ss = s2 * s1, cc = c2 * c1, sc = s2 * c1, cs = c2 * s1;
  double m[4][4];
  m[0][0] = P1;
  m[0][1] = P2 * c1;
  m[0][2] = mirror ? P2 * s1 : -P2 * s1;
  m[0][3] = 0.;
  m[1][0] = P2 * c2;
  m[1][1] = P1 * cc - P3 * ss;
  m[1][2] = mirror ? P1 * cs + P3 * sc : -P1 * cs - P3 * sc;
  m[1][3] = mirror ? -P4 * s2 : P4 * s2;
  m[2][0] = mirror ? -P2 * s2 : P2 * s2;
  m[2][1] = mirror ? -P1 * sc - P3 * cs : P1 * sc + P3 * cs;
  m[2][2] = -P1 * ss + P3 * cc;
  m[2][3] = -P4 * c2;
  m[3][0] = 0.;
  m[3][1] = mirror ? -P4 * s1 : P4 * s1;
  m[3][2] = P4 * c1;
  m[3][3] = P3;
  const double inv = 1. / P1;
  out[0] = (m[0][0] * in[0] + m[0][1] * in[1] + m[0][2] * in[2]) * inv;
  out[1] = (m[1][0] * in[0] + m[1][1] * in[1] + m[1][2] * in[2] +
            m[1][3] * in[3]) *
           inv;
  out[2] = (m[2][0] * in[0] + m[2][1] * in[1] + m[2][2] * in[2] +
            m[2][3] * in[3]) *
           inv;
  out[3] = (m[3][1] * in[1] + m[3][2] * in[2] + m[3][3] * in[3]) * inv;
}

/* White (1979) eqs. 3-5 and the skewed angle of eq. 6 (pc = 0 makes P4 0,
 * but it is evaluated as the reference does) */
static void phase(double mu, double *P1, double *P2, double *P3, double *P4,
                  int degrees) {
  const double mu2 = mu * mu;
  *P1 = M.one_minus_g2 * pow(M.one_plus_g2 - M.two_g * mu, -1.5);
  const double q = 1. / (1. + mu2);
  *P2 = -M.pl * *P1 * (1. - mu2) * q;
  *P3 = 2. * *P1 * mu * q;
  double c;
  if (degrees) { /* scatter_towards, src/DustScattering.cpp:374-379 */
    const double t = acos(mu) * 180. * INV_PI;
    const double f = 3.13 * t * exp(-7. * t / 180.);
    c = cos((t + 1. * f) * M_PI / 180.);
  } else { /* scatter, :138-142 */
    const double t = acos(mu);
    c = cos(t + 1. * 3.13 * t * exp(-7. * t * INV_PI));
  }
  const double c2 = c * c;
  *P4 = -0. * *P1 * (1. - c2) / (1. + c2);
}

/* DustScattering::scatter, src/DustScattering.cpp:41-323 */
static void scatter(stream *s, photon *p) {
  const double t = M.one_minus_g2 / (M.one_minus_g + M.two_g * uniform(s));
  const double mu =
      fmin(1., fmax(-1., M.half_over_g * (M.one_plus_g2 - t * t)));
  if (fabs(mu) == 1.) {
    if (mu == -1.) {
      p->iquv[2] = -p->iquv[2];
      point(p, -p->u[0], -p->u[1], -p->u[2]);
      p->ang[1] = -p->ang[1];
      p->ang[3] = -p->ang[3];
      p->ang[4] = -p->ang[4];
      p->ang[2] += M_PI;
    }
    return;
  }
  const double I0 = p->iquv[0], r = 1. / I0;
  const double in[4] = {1., p->iquv[1] * r, p->iquv[2] * r, p->iquv[3] * r};
  double P1, P2, P3, P4;
  phase(mu, &P1, &P2, &P3, &P4, 0);
  const double smu = sqrt(fmax(0., 1. - mu * mu));
  const double psi = 2. * M_PI * uniform(s);
  const int mirror = psi > M_PI;
  const double a1 = mirror ? 2. * M_PI - psi : psi;
  const double c1 = cos(a1), s1 = sin(a1);
  const double st0 = p->ang[0], ct0 = p->ang[1];
  const double ct = ct0 * mu + st0 * smu * c1;
  double st, s2, c2;
  if (fabs(ct) < 1.) {
    st = fabs(sqrt(1. - ct * ct));
    s2 = s1 * st0 / st;
    c2 = (ct0 - ct * mu) / (st * smu);
  } else {
    st = 0.;
    s2 = 0.;
    c2 = ct >= 1. ? -1. : 1.;
  }
  const double dphi =
      acos(fmin(1., fmax(-1., -c2 * c1 + s2 * s1 * mu)));
  double ph = mirror ? p->ang[2] + dphi : p->ang[2] - dphi;
  if (ph > 2. * M_PI)
    ph -= 2. * M_PI;
  if (ph < 0.)
    ph += 2. * M_PI;
  double out[4];
  mueller(P1, P2, P3, P4, 2. * c1 * c1 - 1., 2. * s1 * c1,
          2. * c2 * c2 - 1., 2. * s2 * c2, mirror, in, out);
  for (int k = 0; k < 4; ++k)
    p->iquv[k] = out[k] * I0;
  p->ang[0] = st;
  p->ang[1] = ct;
  p->ang[2] = ph;
  p->ang[3] = sin(ph);
  p->ang[4] = cos(ph);
  point(p, st * p->ang[4], st * p->ang[3], ct);
}

/* DustScattering::scatter_towards, src/DustScattering.cpp:325-518 */
static double scatter_towards(photon *p) {
  const double mu =
      M.obs[0] * p->u[0] + M.obs[1] * p->u[1] + M.obs[2] * p->u[2];
  if (fabs(mu) == 1.) {
    if (mu == -1.)
      p->iquv[2] = -p->iquv[2];
  } else {
    const double I0 = p->iquv[0], r = 1. / I0;
    const double in[4] = {1., p->iquv[1] * r, p->iquv[2] * r, p->iquv[3] * r};
    double P1, P2, P3, P4;
    phase(mu, &P1, &P2, &P3, &P4, 1);
    const double smu = sqrt(-(mu * mu - 1.));
    const double st0 = p->ang[0], ct0 = p->ang[1];
    double r1;
    if (st0 == 0.) {
      r1 = M_PI;
    } else {
      const double y = sin(p->ang[2] - M.ph - M_PI) * M.st / smu;
      const double x = (M.ct - ct0 * mu) / (st0 * smu);
      r1 = atan2(y, x) + M_PI;
    }
    const int mirror = r1 > M_PI;
    const double a1 = mirror ? 2. * M_PI - r1 : r1;
    const double c1 = cos(a1), s1 = sin(a1);
    double s2, c2;
    if (fabs(M.ct) < 1.) {
      s2 = s1 * st0 / M.st;
      const double den = M.st * smu;
      c2 = ct0 / den - M.ct * mu / den;
    } else {
      s2 = 0.;
      c2 = M.ct >= 1. ? -1. : 1.;
    }
    double out[4];
    mueller(P1, P2, P3, P4, 2. * c1 * c1 - 1., 2. * s1 * c1,
            2. * c2 * c2 - 1., 2. * s2 * c2, mirror, in, out);
    for (int k = 0; k < 4; ++k)
      p->iquv[k] = out[k] * I0;
  }
  point(p, M.obs[0], M.obs[1], M.obs[2]);
  p->ang[0] = M.st;
  p->ang[1] = M.ct;
  p->ang[2] = M.ph;
  p->ang[3] = M.sp;
  p->ang[4] = M.cp;
  return 0.25 * M.one_minus_g2 * pow(M.one_plus_g2 - M.two_g * mu, -1.5) *
         INV_PI;
}

/* ------------------------------------------------------------- image -- */

/* CCDImage::add_photon's projection, src/CCDImage.hpp:242-270 */
int64_t dref_pixel(const double x[3]) {
  double u = x[1] * M.cp - x[0] * M.sp;
  double v = x[2] * M.st - x[1] * M.ct * M.sp - x[0] * M.ct * M.cp;
  if (!(u >= M.ia[0] && v >= M.ia[1]))
    return -1;
  u -= M.ia[0];
  v -= M.ia[1];
  if (!(u < M.is[0] && v < M.is[1]))
    return -1;
  const uint32_t ix = (uint32_t)(M.res[0] * u / M.is[0]);
  const uint32_t iy = (uint32_t)(M.res[1] * v / M.is[1]);
  /* x / side just below 1 can round up to the far edge: no pixel (the
   * reference's vectors would be indexed past their end) */
  if (ix >= (uint32_t)M.res[0] || iy >= (uint32_t)M.res[1])
    return -1;
  return (int64_t)ix * M.res[1] + iy;
}

typedef struct {
  double *image; /* [3][npixel] or NULL */
  double *rows;  /* trace rows or NULL */
  int max_rows, nrows;
  uint64_t steps, scatterings, capped, dropped;
} sink;

static void deposit(sink *k, const double x[3], const double iquv[4],
                    double w) {
  if (k->rows) {
    if (k->nrows < k->max_rows) {
      double *r = k->rows + 8 * k->nrows;
      memcpy(r, x, 3 * sizeof(double));
      memcpy(r + 3, iquv, 4 * sizeof(double));
      r[7] = w;
    }
    ++k->nrows;
  }
  if (k->image) {
    const int64_t px = dref_pixel(x);
    if (px >= 0) {
      const int64_t np = (int64_t)M.res[0] * M.res[1];
      k->image[px] += w * iquv[0];
      k->image[np + px] += w * iquv[1];
      k->image[2 * np + px] += w * iquv[2];
    }
  }
}

/* DustPhotonShootJob::execute for one packet,
 * src/DustPhotonShootJob.hpp:107-164 */
static void packet(uint32_t seed, uint64_t id, sink *k) {
  stream s = {seed, id, 0u};
  photon p;
  if (!emit(&s, &p)) {
    ++k->dropped;
    return;
  }

  photon view = p;
  point(&view, M.obs[0], M.obs[1], M.obs[2]);
  const double direct = 0.25 * exp(-optical_depth(&view, &k->steps, 0, 0)) / M_PI;
  const double unpolarised[4] = {1., 0., 0., 0.};
  deposit(k, p.x, unpolarised, direct);

  const double forced = 1. - exp(-optical_depth(&p, &k->steps, 0, 0));
  double a = 1.;
  int alive = interact(&p, -log(1. - uniform(&s) * forced), &k->steps);
  uint64_t n = 0;
  while (alive) {
    photon peel = p;
    const double hg = scatter_towards(&peel);
    const double tau = optical_depth(&peel, &k->steps, 0, 0);
    a *= M.albedo;
    deposit(k, peel.x, peel.iquv, forced * hg * a * exp(-tau));
    scatter(&s, &p);
    if (++n >= DREF_MAX_SCATTER) {
      ++k->capped;
      break;
    }
    alive = interact(&p, -log(uniform(&s)), &k->steps);
  }
  k->scatterings += n;
}

/* --------------------------------------------------------- the probes -- */
void dref_emit(uint32_t seed, uint64_t first, int64_t n, double *out) {
  for (int64_t k = 0; k < n; ++k) {
    stream s = {seed, first + k, 0u};
    photon p;
    if (!emit(&s, &p)) {
      for (int j = 0; j < 6; ++j)
        out[6 * k + j] = NAN;
      continue;
    }
    memcpy(out + 6 * k, p.x, 3 * sizeof(double));
    memcpy(out + 6 * k + 3, p.u, 3 * sizeof(double));
  }
}

static void load(photon *p, const double *r) {
  point(p, r[0], r[1], r[2]);
  memcpy(p->ang, r + 3, 5 * sizeof(double));
  memcpy(p->iquv, r + 8, 4 * sizeof(double));
  p->x[0] = p->x[1] = p->x[2] = 0.;
}

void dref_scatter(uint32_t seed, uint64_t first, int64_t n, const double *in,
                  double *out) {
  for (int64_t k = 0; k < n; ++k) {
    stream s = {seed, first + k, 0u};
    photon p;
    load(&p, in + 12 * k);
    scatter(&s, &p);
    double *o = out + 12 * k;
    memcpy(o, p.u, 3 * sizeof(double));
    memcpy(o + 3, p.ang, 5 * sizeof(double));
    memcpy(o + 8, p.iquv, 4 * sizeof(double));
  }
}

void dref_scatter_towards(int64_t n, const double *in, double *out) {
  for (int64_t k = 0; k < n; ++k) {
    photon p;
    load(&p, in + 12 * k);
    out[5 * k] = scatter_towards(&p);
    memcpy(out + 5 * k + 1, p.iquv, 4 * sizeof(double));
  }
}

void dref_optical_depth(int64_t n, const double *in, double *out,
                        int32_t max_cells) {
  const int w = 2 + max_cells;
  for (int64_t k = 0; k < n; ++k) {
    photon p;
    memcpy(p.x, in + 6 * k, 3 * sizeof(double));
    point(&p, in[6 * k + 3], in[6 * k + 4], in[6 * k + 5]);
    uint64_t steps = 0;
    out[w * k] = optical_depth(&p, &steps, out + w * k + 2, max_cells);
    out[w * k + 1] = (double)steps;
  }
}

void dref_trace(uint32_t seed, uint64_t first, int64_t n, double *out,
                int32_t max_events) {
  const int w = 4 + 8 * max_events;
  for (int64_t k = 0; k < n; ++k) {
    sink s = {0, out + w * k + 4, max_events, 0, 0, 0, 0, 0};
    packet(seed, first + k, &s);
    out[w * k] = s.nrows;
    out[w * k + 1] = (double)s.scatterings;
    out[w * k + 2] = (double)s.steps;
    out[w * k + 3] = (double)(s.capped + s.dropped);
  }
}

/* the whole run for packets [first, first + n): image [3][nx * ny] added to,
 * counters {steps, scatterings, capped, dropped by the source}; OpenMP
 * threads keep images of their own, summed at the end */
void dref_shoot(uint32_t seed, uint64_t first, int64_t n, double *image,
                uint64_t counters[4]) {
  const int64_t np = 3 * (int64_t)M.res[0] * M.res[1];
  uint64_t steps = 0, scatterings = 0, capped = 0, dropped = 0;
#pragma omp parallel reduction(+ : steps, scatterings, capped, dropped)
  {
    double *mine = calloc(np, sizeof(double));
    sink s = {mine, 0, 0, 0, 0, 0, 0, 0};
#pragma omp for schedule(dynamic, 256)
    for (int64_t k = 0; k < n; ++k)
      packet(seed, first + k, &s);
#pragma omp critical
    for (int64_t i = 0; i < np; ++i)
      image[i] += mine[i];
    free(mine);
    steps += s.steps;
    scatterings += s.scatterings;
    capped += s.capped;
    dropped += s.dropped;
  }
  counters[0] = steps;
  counters[1] = scatterings;
  counters[2] = capped;
  counters[3] = dropped;
}

/* SpiralGalaxyDensityFunction at the cell midpoints
 * (src/SpiralGalaxyDensityFunction.hpp:116-130,
 * src/CartesianDensityGrid.hpp:85-89), as the driver evaluates it: n_0 is
 * the already converted mass density */
void dref_galaxy_density(const double anchor[3], const double sides[3],
                         const int32_t ncell[3], double n_0, double r_ISM,
                         double h_ISM, double *out) {
  const double kpc = 3.086e19;
  double side[3];
  for (int a = 0; a < 3; ++a)
    side[a] = sides[a] / ncell[a];
  const int64_t total = (int64_t)ncell[0] * ncell[1] * ncell[2];
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < total; ++i) {
    const int64_t ix = i / ((int64_t)ncell[1] * ncell[2]);
    const int64_t iy = (i / ncell[2]) % ncell[1];
    const int64_t iz = i % ncell[2];
    const double x = (anchor[0] + side[0] * ix) + 0.5 * side[0];
    const double y = (anchor[1] + side[1] * iy) + 0.5 * side[1];
    const double z = (anchor[2] + side[2] * iz) + 0.5 * side[2];
    const double w = sqrt(x * x + y * y);
    out[i] = (w < 15. * kpc && fabs(z) < 15. * kpc)
                 ? n_0 * exp(-w / r_ISM) * exp(-fabs(z) / h_ISM)
                 : 0.;
  }
}
