/*
 * scattered_cube_reference.c - CPU restatement of the scattered-light line
 * cubes for the tests (include/cmi_gpu.h, "scattered-light line cubes", has
 * the contract). The walk is that of the scattered-light
 * images - scattered_sky_reference.c is included below, and with it
 * scattered_line_reference.c and dust_reference.c, so that their static
 * functions are the ones used: emit_cell, optical_depth, interact, scatter,
 * scatter_towards, towards, optical_depth_to, scatter_towards_point,
 * rotate_to_pole, pixel_of -; what cube mode adds - the packet's Doppler
 * velocity q and variance s2, u and b of an event, the shares f_c of the
 * channels - is restated here operation for operation. Cube mode draws no
 * random number.
 *
 * Built by tests/scattered_cube_lib.py:
 *   gcc -O2 -ffp-contract=off -fopenmp -shared -fPIC
 *       scattered_cube_reference.c -L oracle -lcmio
 * The model is dref_setup's, the source slref_set_field's, the point camera
 * ssref_set_camera's; scube_set_cube sets cube mode.
 */
#include "scattered_sky_reference.c"

#define SCUBE_BOLTZMANN 1.38064852e-23
#define SCUBE_ATOMIC_MASS_UNIT 1.660539040e-27

static struct {
  int32_t nchan;
  double vmin, dv, two_sigma2;
  double *s2;       /* [ncell] */
  double *velocity; /* [3][ncell] or NULL */
  double vobs[3];
  int64_t ncell;
} Q;

static double dot3(const double a[3], const double b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

/* dot3(v_cell, k) */
static double doppler(int64_t cell, const double k[3]) {
  if (!Q.velocity)
    return 0.;
  return (Q.velocity[cell] * k[0] + Q.velocity[Q.ncell + cell] * k[1]) +
         Q.velocity[2 * Q.ncell + cell] * k[2];
}

/* the cell of a scattering */
static int64_t cell_of(const double x[3]) {
  int64_t i[3];
  for (int a = 0; a < 3; ++a) {
    const double c = floor((x[a] - M.anchor[a]) * M.inv_cell[a]);
    i[a] = (int64_t)fmin(fmax(c, 0.), (double)(M.n[a] - 1));
  }
  return (i[0] * M.n[1] + i[1]) * M.n[2] + i[2];
}

static double clamped_erf(double z) {
  return (z >= 6.) ? 1. : ((z > -6.) ? erf(z) : -1.);
}

/* the share of channel c of a Gaussian at u of width b */
static double share(int32_t c, double u, double b) {
  const double e0 = Q.vmin + (double)c * Q.dv;
  const double e1 = Q.vmin + (double)(c + 1) * Q.dv;
  return 0.5 * (clamped_erf((e1 - u) / b) - clamped_erf((e0 - u) / b));
}

void scube_shares(double u, double b, double *f) {
  for (int32_t c = 0; c < Q.nchan; ++c)
    f[c] = share(c, u, b);
}

/* cube mode: the channel axis, the variances (from widths[ncell] if given,
 * else from temperature[ncell] and the atomic weight), the velocities
 * [3][ncell] or NULL, the observer's velocity or NULL */
void scube_set_cube(int32_t nchan, double vmin, double vmax, double sigma_turb,
                    const double *widths, const double *temperature,
                    double atomic_weight, const double *velocity,
                    const double *vobs) {
  int64_t ncell = 1;
  for (int a = 0; a < 3; ++a)
    ncell *= M.n[a];
  free(Q.s2);
  free(Q.velocity);
  Q.ncell = ncell;
  Q.nchan = nchan;
  Q.vmin = vmin;
  Q.dv = (vmax - vmin) / nchan;
  Q.two_sigma2 = 2. * sigma_turb * sigma_turb;
  Q.s2 = malloc(sizeof(double) * ncell);
  for (int64_t c = 0; c < ncell; ++c)
    Q.s2[c] = widths ? 0.5 * widths[c] * widths[c]
                     : SCUBE_BOLTZMANN * temperature[c] /
                               (atomic_weight * SCUBE_ATOMIC_MASS_UNIT) +
                           sigma_turb * sigma_turb;
  Q.velocity = 0;
  if (velocity) {
    Q.velocity = malloc(sizeof(double) * 3 * ncell);
    memcpy(Q.velocity, velocity, sizeof(double) * 3 * ncell);
  }
  for (int a = 0; a < 3; ++a)
    Q.vobs[a] = vobs ? vobs[a] : 0.;
}

typedef struct {
  double *image;   /* [3][npixel] or NULL */
  double *cube;    /* [3][nchan][npixel] or NULL */
  double *squares; /* [2][nchan][npixel]: squared addends of I and their
                      number, or NULL */
  double *rows;    /* trace rows of 10 or NULL */
  int max_rows, nrows;
  int64_t npixel;
  uint64_t steps, scatterings, capped, excluded, outside, events;
} cube_sink;

/* what an event adds; px < 0: nothing but the row */
static void cube_put(cube_sink *y, const double x[3], int64_t px,
                     const double iquv[4], double w, double u, double b) {
  if (y->rows) {
    if (y->nrows < y->max_rows) {
      double *r = y->rows + 10 * y->nrows;
      memcpy(r, x, 3 * sizeof(double));
      memcpy(r + 3, iquv, 4 * sizeof(double));
      r[7] = w;
      r[8] = u;
      r[9] = b;
    }
    ++y->nrows;
  }
  if (!y->image || px < 0)
    return;
  const int64_t np = y->npixel;
  const double a[3] = {w * iquv[0], w * iquv[1], w * iquv[2]};
  for (int k = 0; k < 3; ++k)
    y->image[k * np + px] += a[k];
  ++y->events;
  for (int32_t c = 0; c < Q.nchan; ++c) {
    const double f = share(c, u, b);
    if (f == 0.)
      continue;
    for (int k = 0; k < 3; ++k)
      y->cube[(k * (int64_t)Q.nchan + c) * np + px] += a[k] * f;
    if (y->squares && a[0] * f != 0.) {
      y->squares[c * np + px] += (a[0] * f) * (a[0] * f);
      y->squares[(Q.nchan + c) * np + px] += 1.;
    }
  }
}

/* one event of the parallel camera */
static void event_parallel(cube_sink *y, const photon *p, int scattered,
                           double weight, double albedo, double q, double s2,
                           int64_t cell) {
  photon peel = *p;
  const double vd = doppler(cell, M.obs);
  double w, u, b;
  if (scattered) {
    const double vk = doppler(cell, p->u);
    const double kd = dot3(p->u, M.obs);
    const double hg = scatter_towards(&peel);
    const double tau = optical_depth(&peel, &y->steps, 0, 0);
    w = weight * hg * albedo * exp(-tau);
    u = -(q + (vd - vk));
    b = sqrt(2. * (s2 + Q.two_sigma2 * fmax(0., 1. - kd)));
  } else {
    photon view = *p;
    point(&view, M.obs[0], M.obs[1], M.obs[2]);
    w = 0.25 * exp(-optical_depth(&view, &y->steps, 0, 0)) / M_PI;
    u = -vd;
    b = sqrt(2. * s2);
  }
  cube_put(y, peel.x, y->image ? dref_pixel(peel.x) : -1, peel.iquv, w, u, b);
}

/* one event of the point camera */
static void event_point(cube_sink *y, const photon *p, int scattered,
                        double weight, double albedo, double q, double s2,
                        int64_t cell) {
  photon peel = *p;
  double k[3], r, r2;
  if (!towards(peel.x, k, &r, &r2)) {
    ++y->excluded;
    const double nothing[4] = {0., 0., 0., 0.};
    cube_put(y, peel.x, -1, nothing, 0., 0., 0.);
    return;
  }
  const double vd = doppler(cell, k);
  const double od = dot3(Q.vobs, k);
  double W, u, b;
  if (scattered) {
    const double vk = doppler(cell, p->u);
    const double kd = dot3(p->u, k);
    const double hg = scatter_towards_point(&peel, k);
    const double tau = optical_depth_to(&peel, r, &y->steps);
    if (!K.pole_is_z)
      rotate_to_pole(k, peel.iquv);
    W = weight * hg * albedo * exp(-tau);
    u = -((q + (vd - vk)) - od);
    b = sqrt(2. * (s2 + Q.two_sigma2 * fmax(0., 1. - kd)));
  } else {
    photon view = peel;
    point(&view, k[0], k[1], k[2]);
    W = 0.25 * exp(-optical_depth_to(&view, r, &y->steps)) / M_PI;
    u = -(vd - od);
    b = sqrt(2. * s2);
  }
  const double w = W / r2;
  int64_t px = -1;
  if (y->image) {
    px = pixel_of(k);
    if (px < 0)
      ++y->outside;
  }
  cube_put(y, peel.x, px, peel.iquv, w, u, b);
}

static void cube_event(cube_sink *y, int camera_is_point, const photon *p,
                       int scattered, double weight, double albedo, double q,
                       double s2, int64_t cell) {
  if (!camera_is_point)
    event_parallel(y, p, scattered, weight, albedo, q, s2, cell);
  else if (scattered || K.direct_light)
    event_point(y, p, scattered, weight, albedo, q, s2, cell);
}

/* line_packet() / sky_packet() in cube mode */
static void cube_packet(uint32_t seed, uint64_t id, int camera_is_point,
                        cube_sink *y) {
  stream s = {seed, id, 0u};
  photon p;
  const int64_t ecell = emit_cell(&s, &p);
  double q = doppler(ecell, p.u);
  double s2 = Q.s2[ecell];

  cube_event(y, camera_is_point, &p, 0, 1., 1., q, s2, ecell);

  const double forced = 1. - exp(-optical_depth(&p, &y->steps, 0, 0));
  double a = 1.;
  int alive = interact(&p, -log(1. - uniform(&s) * forced), &y->steps);
  uint64_t n = 0;
  while (alive) {
    a *= M.albedo;
    const int64_t scell = cell_of(p.x);
    cube_event(y, camera_is_point, &p, 1, forced, a, q, s2, scell);
    const double k[3] = {p.u[0], p.u[1], p.u[2]};
    scatter(&s, &p);
    q += doppler(scell, p.u) - doppler(scell, k);
    s2 += Q.two_sigma2 * fmax(0., 1. - dot3(k, p.u));
    if (++n >= DREF_MAX_SCATTER) {
      ++y->capped;
      break;
    }
    alive = interact(&p, -log(uniform(&s)), &y->steps);
  }
  y->scatterings += n;
}

static int64_t camera_pixels(int camera_is_point) {
  return camera_is_point ? (int64_t)K.nlon * K.nlat
                         : (int64_t)M.res[0] * M.res[1];
}

/* rows {events, scatterings, steps, capped, rows[max_events][10]} */
void scube_trace(int32_t camera_is_point, uint32_t seed, uint64_t first,
                 int64_t n, double *out, int32_t max_events) {
  const int w = 4 + 10 * max_events;
  for (int64_t k = 0; k < n; ++k) {
    cube_sink y;
    memset(&y, 0, sizeof y);
    y.rows = out + w * k + 4;
    y.max_rows = max_events;
    cube_packet(seed, first + k, camera_is_point, &y);
    out[w * k] = y.nrows;
    out[w * k + 1] = (double)y.scatterings;
    out[w * k + 2] = (double)y.steps;
    out[w * k + 3] = (double)y.capped;
  }
}

/* the whole run: image [3][npixel], cube [3][nchan][npixel], squares
 * [2][nchan][npixel] (may be NULL), all added to; counters {steps, scatterings,
 * capped, excluded, outside, events that reached a pixel} */
void scube_shoot(int32_t camera_is_point, uint32_t seed, uint64_t first,
                 int64_t n, double *image, double *cube, double *squares,
                 uint64_t counters[6]) {
  const int64_t np = camera_pixels(camera_is_point);
  const int64_t ni = 3 * np, nc = 3 * Q.nchan * np, ns = 2 * Q.nchan * np;
  uint64_t steps = 0, scatterings = 0, capped = 0, excluded = 0, outside = 0,
           events = 0;
#pragma omp parallel reduction(+ : steps, scatterings, capped, excluded, outside, events)
  {
    double *mine = calloc(ni + nc + ns, sizeof(double));
    cube_sink y;
    memset(&y, 0, sizeof y);
    y.image = mine;
    y.cube = mine + ni;
    y.squares = squares ? mine + ni + nc : 0;
    y.npixel = np;
#pragma omp for schedule(dynamic, 256)
    for (int64_t k = 0; k < n; ++k)
      cube_packet(seed, first + k, camera_is_point, &y);
#pragma omp critical
    {
      for (int64_t i = 0; i < ni; ++i)
        image[i] += mine[i];
      for (int64_t i = 0; i < nc; ++i)
        cube[i] += mine[ni + i];
      if (squares)
        for (int64_t i = 0; i < ns; ++i)
          squares[i] += mine[ni + nc + i];
    }
    free(mine);
    steps += y.steps;
    scatterings += y.scatterings;
    capped += y.capped;
    excluded += y.excluded;
    outside += y.outside;
    events += y.events;
  }
  counters[0] = steps;
  counters[1] = scatterings;
  counters[2] = capped;
  counters[3] = excluded;
  counters[4] = outside;
  counters[5] = events;
}
