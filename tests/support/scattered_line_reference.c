/*
 * scattered_line_reference.c - CPU restatement of the scattered-light line
 * images for the tests: the cell-luminosity source (its tables, its selection
 * rule, its draws) and the packet's life after emission, which is the dust
 * restatement's (dust_reference.c, included below so that its static
 * functions are the ones used: optical_depth, interact, scatter_towards,
 * scatter, deposit). The device path (cmacionize_amd/csrc/device_dust.h,
 * dust_kernels.h, line_image_kernels.h) is checked against it on the same
 * random streams.
 *
 * Built by the test that uses it, as dust_reference.c is:
 *   gcc -O2 -ffp-contract=off -fopenmp -shared -fPIC
 *       scattered_line_reference.c -L oracle -lcmio
 * The model (grid, dust, image) is dref_setup's, with x_H = 1 and kappa = the
 * cross section per hydrogen nucleus: the opacity is then n sigma.
 *
 * Tables (the contract): blocks of SLREF_BLOCK = 256
 * consecutive cells; C[c] the running sum of w within c's block, cell by
 * cell from 0; B[b] the running sum of the block totals, block by block.
 */
#include "dust_reference.c"

#define SLREF_BLOCK 256

static struct {
  int64_t ncell, nblock;
  double *C, *B;
} S;

/* 0: built; 1: a weight is negative or not finite; 2: nothing emits */
int slref_set_field(const double *w, int64_t ncell) {
  free(S.C);
  free(S.B);
  S.ncell = ncell;
  S.nblock = (ncell + SLREF_BLOCK - 1) / SLREF_BLOCK;
  S.C = malloc(sizeof(double) * ncell);
  S.B = malloc(sizeof(double) * S.nblock);
  if (!S.C || !S.B)
    return 3;
  for (int64_t c = 0; c < ncell; ++c)
    if (!(w[c] >= 0.) || !isfinite(w[c]))
      return 1;
  double total = 0.;
  for (int64_t b = 0; b < S.nblock; ++b) {
    const int64_t lo = b * SLREF_BLOCK;
    const int64_t hi = lo + SLREF_BLOCK < ncell ? lo + SLREF_BLOCK : ncell;
    double sum = 0.;
    for (int64_t c = lo; c < hi; ++c) {
      sum += w[c];
      S.C[c] = sum;
    }
    total += sum;
    S.B[b] = total;
  }
  return total > 0. ? 0 : 2;
}

/* total = V_cell B[last]; either table may be NULL */
void slref_get_tables(double *total, double *B, double *C) {
  if (total)
    *total = M.cell[0] * M.cell[1] * M.cell[2] * S.B[S.nblock - 1];
  if (B)
    memcpy(B, S.B, sizeof(double) * S.nblock);
  if (C)
    memcpy(C, S.C, sizeof(double) * S.ncell);
}

/* first index in [lo, hi) with a[i] > x, or hi */
static int64_t first_above(const double *a, int64_t lo, int64_t hi, double x) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] > x)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

/* first index in [lo, hi) with a[i] == a[hi - 1] */
static int64_t first_equal_last(const double *a, int64_t lo, int64_t hi) {
  const double last = a[hi - 1];
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] == last)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

/* the selection rule for the offset t = u B[last] */
static int64_t select_cell(double t) {
  int64_t b = first_above(S.B, 0, S.nblock, t);
  if (b == S.nblock) /* u B[last] rounded up to B[last] */
    b = first_equal_last(S.B, 0, S.nblock);
  const double r = t - (b > 0 ? S.B[b - 1] : 0.);
  const int64_t lo = b * SLREF_BLOCK;
  const int64_t hi = lo + SLREF_BLOCK < S.ncell ? lo + SLREF_BLOCK : S.ncell;
  int64_t k = first_above(S.C, lo, hi, r);
  if (k == hi)
    k = first_equal_last(S.C, lo, hi);
  return k;
}

void slref_select(int64_t n, const double *u, int64_t *cells) {
  const double total = S.B[S.nblock - 1];
  for (int64_t i = 0; i < n; ++i)
    cells[i] = select_cell(u[i] * total);
}

/* the draws of a packet up to the first march: cell selector; x, y, z;
 * cos theta, phi */
static int64_t emit_cell(stream *s, photon *p) {
  const int64_t cell = select_cell(uniform(s) * S.B[S.nblock - 1]);
  const int64_t i[3] = {cell / ((int64_t)M.n[1] * M.n[2]),
                        (cell / M.n[2]) % M.n[1], cell % M.n[2]};
  for (int a = 0; a < 3; ++a)
    p->x[a] = (M.anchor[a] + M.cell[a] * i[a]) + uniform(s) * M.cell[a];
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
  return cell;
}

/* per-pixel statistics of I for the tests: sum of squared contributions and
 * their number */
typedef struct {
  sink k;
  double *squares, *hits;
} stat_sink;

static void put(stat_sink *t, const double x[3], const double iquv[4],
                double w) {
  deposit(&t->k, x, iquv, w);
  if (t->squares) {
    const int64_t px = dref_pixel(x);
    if (px >= 0 && w * iquv[0] != 0.) {
      t->squares[px] += (w * iquv[0]) * (w * iquv[0]);
      t->hits[px] += 1.;
    }
  }
}

/* dust_reference.c's packet() with the cell source in place of the galaxy */
static void line_packet(uint32_t seed, uint64_t id, stat_sink *t) {
  sink *k = &t->k;
  stream s = {seed, id, 0u};
  photon p;
  (void)emit_cell(&s, &p);

  photon view = p;
  point(&view, M.obs[0], M.obs[1], M.obs[2]);
  const double direct =
      0.25 * exp(-optical_depth(&view, &k->steps, 0, 0)) / M_PI;
  const double unpolarised[4] = {1., 0., 0., 0.};
  put(t, p.x, unpolarised, direct);

  const double forced = 1. - exp(-optical_depth(&p, &k->steps, 0, 0));
  double a = 1.;
  int alive = interact(&p, -log(1. - uniform(&s) * forced), &k->steps);
  uint64_t n = 0;
  while (alive) {
    photon peel = p;
    const double hg = scatter_towards(&peel);
    const double tau = optical_depth(&peel, &k->steps, 0, 0);
    a *= M.albedo;
    put(t, peel.x, peel.iquv, forced * hg * a * exp(-tau));
    scatter(&s, &p);
    if (++n >= DREF_MAX_SCATTER) {
      ++k->capped;
      break;
    }
    alive = interact(&p, -log(uniform(&s)), &k->steps);
  }
  k->scatterings += n;
}

/* rows {cell, pos[3], dir[3]} */
void slref_emit(uint32_t seed, uint64_t first, int64_t n, double *out) {
  for (int64_t k = 0; k < n; ++k) {
    stream s = {seed, first + k, 0u};
    photon p;
    out[7 * k] = (double)emit_cell(&s, &p);
    memcpy(out + 7 * k + 1, p.x, 3 * sizeof(double));
    memcpy(out + 7 * k + 4, p.u, 3 * sizeof(double));
  }
}

/* rows as dref_trace's */
void slref_trace(uint32_t seed, uint64_t first, int64_t n, double *out,
                 int32_t max_events) {
  const int w = 4 + 8 * max_events;
  for (int64_t k = 0; k < n; ++k) {
    stat_sink t = {{0, out + w * k + 4, max_events, 0, 0, 0, 0, 0}, 0, 0};
    line_packet(seed, first + k, &t);
    out[w * k] = t.k.nrows;
    out[w * k + 1] = (double)t.k.scatterings;
    out[w * k + 2] = (double)t.k.steps;
    out[w * k + 3] = (double)(t.k.capped + t.k.dropped);
  }
}

/* the whole run as dref_shoot's; squares and hits ([nx * ny] each, added to)
 * may be NULL */
void slref_shoot(uint32_t seed, uint64_t first, int64_t n, double *image,
                 double *squares, double *hits, uint64_t counters[4]) {
  const int64_t npix = (int64_t)M.res[0] * M.res[1];
  const int64_t np = 3 * npix;
  uint64_t steps = 0, scatterings = 0, capped = 0, dropped = 0;
#pragma omp parallel reduction(+ : steps, scatterings, capped, dropped)
  {
    double *mine = calloc(np + 2 * npix, sizeof(double));
    stat_sink t = {{mine, 0, 0, 0, 0, 0, 0, 0},
                   squares ? mine + np : 0,
                   squares ? mine + np + npix : 0};
#pragma omp for schedule(dynamic, 256)
    for (int64_t k = 0; k < n; ++k)
      line_packet(seed, first + k, &t);
#pragma omp critical
    {
      for (int64_t i = 0; i < np; ++i)
        image[i] += mine[i];
      if (squares)
        for (int64_t i = 0; i < npix; ++i) {
          squares[i] += mine[np + i];
          hits[i] += mine[np + npix + i];
        }
    }
    free(mine);
    steps += t.k.steps;
    scatterings += t.k.scatterings;
    capped += t.k.capped;
    dropped += t.k.dropped;
  }
  counters[0] = steps;
  counters[1] = scatterings;
  counters[2] = capped;
  counters[3] = dropped;
}
