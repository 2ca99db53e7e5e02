/*
 * lyman_alpha_kernels.h - Lyman-alpha transfer: Monte Carlo packets that
 * scatter resonantly off H I and off dust, with the redistribution in
 * frequency at every scattering (include/cmi_gpu.h, "Lyman alpha", has the
 * contract; DESIGN.md 4.17 the derivation). The source, the cameras, the
 * phase functions of the dust and the per-packet random stream are those of
 * the scattered-light cubes (device_dust.h, dust_cube_kernels.h); what is
 * new is a march whose opacity depends on the packet's frequency: one Voigt
 * profile per cell crossing from a 64-byte record per cell, and an atom whose
 * velocity is drawn at every hydrogen scattering.
 *
 * dot3(a, b) = (a_x b_x + a_y b_y) + a_z b_z, no contraction, as in
 * dust_cube_kernels.h. The geometry of a crossing is GridRay::step (ray_walk.h:
 * the EXACT marcher's arithmetic); a walk that ends inside a cell backs off
 * along the segment exactly as dda_step does.
 *
 * Mapping. A packet's life is a state (LyaState) that lya_begin creates and
 * lya_event advances by one event: the species, the atom, the peel-off
 * marches of every view, the new direction and the walk to the next event. A
 * packet's numbers depend on its id alone - its random stream is keyed by it
 * -, not on the lane that ran it, so the kernel is free to map packets to
 * lanes either way. As built, a lane keeps the packet of its thread index to
 * the end. With -DCMI_LYA_EVENT_LOOP a wave loops over events instead: a lane
 * whose packet has left claims the next packet id from a device counter. It
 * pays only where a launch holds several times more packets than the device
 * has lanes, which the bounded launches do not: measured 8 % slower (DESIGN.md
 * 4.17), it is kept as `make variant`.
 *
 * Device image [view][pixel] and cube [view][pixel][channel] (Stokes I only,
 * the channel fastest; dust_cube_reorder_kernel turns a view into the ABI's
 * [channel][pixel]). An event is a delta in velocity: one atomic into the
 * image and one into the cube per event and view.
 *
 * The radiation field (include/cmi_gpu.h, "Lyman alpha radiation field";
 * DESIGN.md 4.18). With FIELD the walk also tallies, per cell, one 64-byte row
 * {L, S_H, S_d, G_x, G_y, G_z, N_H, N_d}: the first flight as an expected
 * value along the march that finds tau_max, every later walk by its track
 * length, the events as collision estimators. A lane's adds of one crossing
 * land in one cache line. FIELD is a compile-time switch of the shoot kernel
 * and of the two marches; without it they are the code they were, and the
 * peel-off marches and the probes never tally.
 */
#ifndef CMI_LYMAN_ALPHA_KERNELS_H
#define CMI_LYMAN_ALPHA_KERNELS_H

#include "dust_cube_kernels.h"
#include "ray_walk.h"

#define CMI_LYA_LAMBDA0 1215.67e-10
#define CMI_LYA_A21 6.265e8
/* the atomic weight the line cubes use for H alpha's width */
#define CMI_LYA_HYDROGEN_WEIGHT 1.00794
/* exp(-x^2) is left out of H from this x^2 on: below 2e-28, against a wing of
 * at least a / (sqrt(pi) x^2) > 1e-7 for every a the records can hold */
#define CMI_LYA_EXP_CUT 64.
/* attempts of the atom sampler's rejection loop after which the last
 * candidate is taken (a NaN frequency would otherwise never leave it) */
#define CMI_LYA_MAX_ATTEMPTS 1000000u

/* one cell: line-centre opacity, 1 / b, Voigt parameter, dust opacity, bulk
 * velocity, and the H I density the opacity was built from (the walk does not
 * read it; lya_coupling_kernel does); one half cache line */
struct alignas(64) LyaRecord {
  double kappa0, inv_b, a, kappa_d;
  double v[3];
  double n_HI;
};

/* what a Lyman-alpha launch reads beyond the dust kernels' arguments */
struct LyaDev {
  const LyaRecord *records;
  double x_crit, x_crit2; /* core skipping: x_crit and its square */
  uint32_t max_scatter;
  int32_t nchan;
  double vmin, dv;
  int64_t npixel; /* of one view */
  double *image;  /* [nviews][npixel] */
  double *cube;   /* [nviews][npixel][nchan] */
};

struct LyaCountersDev {
  unsigned long long nsteps;      /* cell crossings, all marches */
  unsigned long long nhydrogen;   /* scatterings off H I */
  unsigned long long ndust;       /* scatterings off dust */
  unsigned long long nrejections; /* rejected candidates of the atom sampler */
  unsigned long long natomics;    /* fp64 atomics into image and cube */
  unsigned long long ncapped;     /* packets stopped at max_scatter */
  unsigned long long npackets;
};

/* a trace's rows of 12: {pos[3], k[3], q, weight, species, u, u_par, x}; the
 * direction and q are the incoming ones, species 0 is the direct light, 1
 * hydrogen, 2 dust, weight the addend to the selected view and u its velocity
 * (u_par and x are 0 where no atom was drawn) */
#define CMI_LYA_TRACE_ROW 12
struct LyaTrace {
  double *rows;
  int max_events, n;
};

/* a packet between two trips of the event loop */
struct LyaState {
  PacketRng rng;
  DustPhoton p;
  double q;      /* lab-frame shift as a velocity, positive = blue */
  double forced; /* weight of the forced first interaction */
  double albedo; /* product of the dust albedos so far */
  uint32_t nscatter;
  bool alive;
};

/* the row of a cell of the radiation field */
#define CMI_LYA_FIELD_ROW 8
enum {
  LYA_FIELD_L = 0,
  LYA_FIELD_S_H = 1,
  LYA_FIELD_S_D = 2,
  LYA_FIELD_G = 3,
  LYA_FIELD_N_H = 6,
  LYA_FIELD_N_D = 7
};

/* what a launch with the field on reads beyond LyaDev: the kernel's last
 * argument, absent without the field */
struct LyaFieldDev {
  double *rows;      /* [ncell][8], 64-byte aligned */
  double momentum_d; /* 1 - albedo g: the share of its momentum that a packet
                        leaves with the dust */
};

/* the tally of a walk: the rows, the dust's momentum share and the weight of
 * the flight; nothing at all without the field */
template <bool FIELD> struct LyaTally {};
template <> struct LyaTally<true> {
  double *rows;
  double momentum_d;
  double W;
};

/* E(t) = (1 - exp(-t)) / t, 1 at t = 0: the mean of exp(-t') over a crossing
 * of depth t */
__device__ __forceinline__ double lya_mean_transmission(double t) {
  return (t > 0.) ? -expm1(-t) / t : 1.;
}

/* a flight of effective length len (weight included) along k through `cell`,
 * where hydrogen's opacity is kH and the dust's kd */
__device__ __forceinline__ void lya_tally_flight(const LyaTally<true> &t,
                                                 int64_t cell, double len,
                                                 double kH, double kd,
                                                 const double k[3]) {
  double *row = t.rows + CMI_LYA_FIELD_ROW * cell;
  const double push = len * (kH + kd * t.momentum_d);
  atomicAdd(row + LYA_FIELD_L, len);
  atomicAdd(row + LYA_FIELD_S_H, len * kH);
  atomicAdd(row + LYA_FIELD_S_D, len * kd);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    atomicAdd(row + LYA_FIELD_G + a, push * k[a]);
}

struct LyaRecordArgs {
  const double *number_density, *x_H; /* the engine's cells */
  const double *n_HI, *temperature;   /* the caller's, or null / the cells' */
  const double *velocity;             /* [3][ncell] or null */
  double sigma_turb, sigma_d;
  int64_t ncell;
  LyaRecord *out;
  unsigned int *ninvalid;
};

/* the records of the cells as they are; a cell whose b is not positive and
 * finite or whose densities are negative or not finite is counted */
__global__ void __launch_bounds__(256) lya_record_kernel(const LyaRecordArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned int bad = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.ncell;
       c += stride) {
    const double n_H = a.number_density[c];
    const double n_HI = a.n_HI ? a.n_HI[c] : n_H * a.x_H[c];
    const double T = a.temperature[c];
    const double s2 = CMI_BOLTZMANN * T /
                          (CMI_LYA_HYDROGEN_WEIGHT * CMI_ATOMIC_MASS_UNIT) +
                      a.sigma_turb * a.sigma_turb;
    const double b = sqrt(2. * s2);
    bad += (b > 0. && b < HUGE_VAL && n_HI >= 0. && n_HI < HUGE_VAL &&
            n_H >= 0. && n_H < HUGE_VAL)
               ? 0u
               : 1u;
    LyaRecord r;
    r.kappa0 = n_HI *
               (3. * CMI_LYA_LAMBDA0 * CMI_LYA_LAMBDA0 * CMI_LYA_LAMBDA0 *
                CMI_LYA_A21 / (8. * M_PI * sqrt(M_PI))) /
               b;
    r.inv_b = 1. / b;
    r.a = CMI_LYA_A21 * CMI_LYA_LAMBDA0 / (4. * M_PI * b);
    r.kappa_d = n_H * a.sigma_d;
    for (int k = 0; k < 3; ++k)
      r.v[k] = a.velocity ? a.velocity[k * a.ncell + c] : 0.;
    r.n_HI = n_HI;
    a.out[c] = r;
  }
  for (int off = 32; off > 0; off >>= 1)
    bad += __shfl_down(bad, off, 64);
  if (threadIdx.x % 64 == 0 && bad)
    atomicAdd(a.ninvalid, bad);
}

/* the wing term Q of H(a, x) = sqrt(pi) Q + exp(-x^2) from x^2 (Tasitsiomi
 * 2006); the absorption spectra (absorption_kernels.h) use it too */
__device__ __forceinline__ double lya_voigt_wing(double a, double x2) {
  const double z = (x2 - 0.855) / (x2 + 3.42);
  double Q = 0.;
  if (z > 0.)
    Q = (1. + 21. / x2) * a / (M_PI * (x2 + 1.)) *
        (z * (0.1117 + z * (4.421 + z * (-9.207 + 5.674 * z))));
  return Q;
}

/* H(a, x) from x^2: the approximation of the contract (Tasitsiomi 2006) */
__device__ __forceinline__ double lya_voigt(double a, double x2) {
  const double Q = lya_voigt_wing(a, x2);
  const double core = (x2 < CMI_LYA_EXP_CUT) ? exp(-x2) : 0.;
  return sqrt(M_PI) * Q + core;
}

/* kappa(x) of a packet of shift q flying along k in the cell of record r; kH
 * receives hydrogen's share, x the frequency in Doppler widths */
__device__ __forceinline__ double lya_opacity(const LyaRecord &r, double q,
                                              const double k[3], double &kH,
                                              double &x) {
  x = (q - dust_dot3(r.v, k)) * r.inv_b;
  kH = r.kappa0 * lya_voigt(r.a, x * x);
  return kH + r.kappa_d;
}

/* a walk from pos along dir: the cell the reference's get_cell_indices gives
 * (a truncating conversion) */
__device__ __forceinline__ void lya_start(const GridDev &g, GridRay &r,
                                          const double pos[3],
                                          const double dir[3],
                                          const double inv_dir[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.pos[a] = pos[a];
    r.d[a] = dir[a];
    r.inv_d[a] = inv_dir[a];
    r.index[a] = (int32_t)((pos[a] - g.anchor[a]) * g.inv_cellside[a]);
  }
}

/* the optical depth to the box edge of a packet of shift q. With FIELD it is
 * the first flight of a packet and tallies its expected value: a crossing of
 * length ds that begins at the depth tau counts ds exp(-tau) E(ds kappa), the
 * length that the light of weight t.W still in flight covers in it */
template <bool FIELD>
__device__ __noinline__ double lya_integrate(const GridDev &g,
                                             const LyaRecord *__restrict__ rec,
                                             const double pos[3],
                                             const double dir[3],
                                             const double inv_dir[3], double q,
                                             unsigned long long &nsteps,
                                             LyaTally<FIELD> t = {}) {
  GridRay r;
  lya_start(g, r, pos, dir, inv_dir);
  double tau = 0.;
  int n = 0;
  while (r.inside(g)) {
    const int64_t cell = r.cell(g);
    const LyaRecord c = rec[cell];
    const double ds = r.step(g);
    double kH, x;
    const double dtau = ds * lya_opacity(c, q, dir, kH, x);
    if constexpr (FIELD)
      lya_tally_flight(t, cell,
                       t.W * ((ds * exp(-tau)) * lya_mean_transmission(dtau)),
                       kH, c.kappa_d, dir);
    tau += dtau;
    ++n;
  }
  nsteps += n;
  return tau;
}

/* moves the photon until the optical depth is used up; false: it left the
 * box, or no step was taken (dust_interact's contract). With FIELD every
 * crossing tallies t.W times the length flown in it (the backed-off length in
 * the last one) */
template <bool FIELD>
__device__ __noinline__ bool lya_interact(const GridDev &g,
                                          const LyaRecord *__restrict__ rec,
                                          DustPhoton &p, double q, double tau,
                                          unsigned long long &nsteps,
                                          LyaTally<FIELD> t = {}) {
  GridRay r;
  lya_start(g, r, p.pos, p.dir, p.inv_dir);
  int n = 0;
  while (r.inside(g) && tau > 0.) {
    const int64_t cell = r.cell(g);
    const LyaRecord c = rec[cell];
    const double from[3] = {r.pos[0], r.pos[1], r.pos[2]};
    const int32_t in[3] = {r.index[0], r.index[1], r.index[2]};
    const double ds = r.step(g);
    double kH, x;
    const double tau_cell = ds * lya_opacity(c, q, p.dir, kH, x);
    tau -= tau_cell;
    double flown = ds;
    if (tau < 0.) {
      const double back = ds * tau / tau_cell;
      flown = ds + back;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        r.pos[a] = from[a] + (r.pos[a] - from[a]) * (ds + back) / ds;
        r.index[a] = in[a];
      }
    }
    if constexpr (FIELD)
      lya_tally_flight(t, cell, t.W * flown, kH, c.kappa_d, p.dir);
    ++n;
  }
  nsteps += n;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    p.pos[a] = r.pos[a];
  return n > 0 && r.inside(g);
}

/* the separation point of the atom sampler for x >= 0: Laursen et al.
 * (2009)'s up to their core-wing transition x_cw(a), then x - 0.5, at most 4;
 * not below 0. It changes the acceptance rate only: at least 0.046 for |x| <=
 * 12 and a of 1.5e-4 to 1.5e-2, about 1.8 / |x| far in the wing */
__device__ __forceinline__ double lya_u0(double x, double a) {
  const double la = log10(a);
  const double x_cw = 1.59 - 0.60 * la - 0.03 * la * la;
  if (x < 0.2)
    return 0.;
  if (x < x_cw)
    return fmax(0., x - 0.01 * pow(a, 1. / 6.) * exp(1.2 * x));
  return fmin(4., fmax(0., x - 0.5));
}

/* the atom's velocity along k in Doppler widths, from f(u) ~ exp(-u^2) /
 * ((x - u)^2 + a^2) by the rejection method of Zheng & Miralda-Escude (2002):
 * three uniforms per attempt {region, angle, acceptance} */
__device__ __noinline__ double lya_sample_parallel(double x, double a,
                                                   PacketRng &rng,
                                                   unsigned long long &nrej) {
  const double ax = fabs(x);
  const double u0 = lya_u0(ax, a);
  const double e0 = exp(-(u0 * u0));
  const double th0 = atan((u0 - ax) / a);
  const double p =
      (th0 + M_PI_2) / ((1. - e0) * th0 + (1. + e0) * M_PI_2);
  double u = 0.;
  unsigned int rejected = 0;
  for (unsigned int attempt = 0; attempt < CMI_LYA_MAX_ATTEMPTS; ++attempt) {
    const double R1 = rng.next();
    const double R2 = rng.next();
    const double R3 = rng.next();
    bool accept;
    if (R1 <= p) {
      const double th = -M_PI_2 + R2 * (th0 + M_PI_2);
      u = a * tan(th) + ax;
      accept = R3 <= exp(-(u * u));
    } else {
      const double th = th0 + R2 * (M_PI_2 - th0);
      u = a * tan(th) + ax;
      accept = R3 <= exp(-(u * u)) / e0;
    }
    if (accept)
      break;
    ++rejected;
  }
  nrej += rejected;
  return (x < 0.) ? -u : u;
}

/* an isotropic direction from two uniforms, as dust_emit_cells sets it */
__device__ __forceinline__ void lya_isotropic(PacketRng &rng, DustPhoton &p) {
  const double cost = 2. * rng.next() - 1.;
  const double sint = sqrt(fmax(1. - cost * cost, 0.));
  const double phi = 2. * M_PI * rng.next();
  const double cosp = cos(phi);
  const double sinp = sin(phi);
  const double dir[3] = {sint * cosp, sint * sinp, cost};
  dust_set_direction(p, dir);
  p.par[0] = sint;
  p.par[1] = cost;
  p.par[2] = phi;
  p.par[3] = sinp;
  p.par[4] = cosp;
}

/* the channel of the velocity u: e_c <= u < e_{c+1} with e_c = vmin + c dv
 * (the lower edge inclusive, the line cubes' rule for b == 0); -1 outside */
__device__ __forceinline__ int32_t lya_channel(const LyaDev &l, double u) {
  const double f = floor((u - l.vmin) / l.dv);
  if (!(f >= -1.) || !(f <= (double)l.nchan))
    return -1;
  int32_t c = (int32_t)f;
  if (u < l.vmin + (double)c * l.dv)
    --c;
  else if (u >= l.vmin + (double)(c + 1) * l.dv)
    ++c;
  return (c >= 0 && c < l.nchan) ? c : -1;
}

/* one event towards the camera dv, view `view`: the direct light (species 0)
 * or the peel-off at a scattering off hydrogen (1) or dust (2) of the photon p
 * of shift q; w is the velocity of the scatterer (the emitting atom, the
 * scattering atom, the cell's bulk velocity) and W the packet's weight */
__device__ __noinline__ void lya_peel(const GridDev &g, const DustDev &dv,
                                      const LyaDev &l, int view,
                                      const DustPhoton &p, int species,
                                      double q, const double w[3], double W,
                                      double u_par, double x,
                                      LyaCountersDev &c, LyaTrace &tr) {
  DustPhoton peel = p;
  const double wd = dust_dot3(w, dv.obs_dir);
  double factor, q_d;
  if (species == 2) {
    factor = dust_scatter_towards(dv, peel);
    q_d = q + (wd - dust_dot3(w, p.dir));
  } else {
    factor = 0.25 / M_PI;
    q_d = (species == 0) ? wd : q + (wd - dust_dot3(w, p.dir));
  }
  const double tau = lya_integrate<false>(g, l.records, p.pos, dv.obs_dir,
                                          dv.obs_inv_dir, q_d, c.nsteps);
  const double addend = ((W * factor) * exp(-tau)) * peel.stokes[0];
  const double u = -q_d;
  if (tr.rows) {
    if (tr.n < tr.max_events) {
      double *r = tr.rows + CMI_LYA_TRACE_ROW * tr.n;
      for (int a = 0; a < 3; ++a) {
        r[a] = p.pos[a];
        r[3 + a] = p.dir[a];
      }
      r[6] = q;
      r[7] = addend;
      r[8] = (double)species;
      r[9] = u;
      r[10] = u_par;
      r[11] = x;
    }
    ++tr.n;
    return;
  }
  const int64_t pixel = dust_pixel(dv, p.pos);
  if (pixel < 0 || addend == 0.)
    return;
  const int64_t at = (int64_t)view * l.npixel + pixel;
  atomicAdd(l.image + at, addend);
  ++c.natomics;
  const int32_t ch = lya_channel(l, u);
  if (ch >= 0) {
    atomicAdd(l.cube + at * l.nchan + ch, addend);
    ++c.natomics;
  }
}

/* lya_peel for every view of the camera, in the order 0..K-1 */
template <int CAMERA>
__device__ __forceinline__ void
lya_peel_views(const GridDev &g, const DustDev &d,
               const DustCamera<CAMERA> &cam, const LyaDev &l,
               const DustPhoton &p, int species, double q, const double w[3],
               double W, double u_par, double x, DustDev &dv,
               LyaCountersDev &c, LyaTrace &tr) {
  if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS) {
    for (int v = 0; v < cam.nviews; ++v) {
      dust_select_view(cam, v, dv);
      lya_peel(g, dv, l, v, p, species, q, w, W, u_par, x, c, tr);
    }
  } else {
    lya_peel(g, d, l, 0, p, species, q, w, W, u_par, x, c, tr);
  }
}

/* a new packet: the cell source's draws, the emitting atom (two Box-Muller
 * pairs, the second's sine unused), the direct light, the forced first
 * interaction and the walk to it. The march for tau_max tallies the first
 * flight with weight 1, the light that leaves unscattered included; the forced
 * walk that follows tallies nothing */
template <int CAMERA, bool FIELD>
__device__ __forceinline__ void
lya_begin(const GridDev &g, const DustDev &d, const CellSourceDev &src,
          const DustCamera<CAMERA> &cam, const LyaDev &l, uint32_t seed,
          uint64_t id, LyaState &s, DustDev &dv, LyaCountersDev &c,
          LyaTrace &tr, LyaTally<FIELD> &t) {
  s.rng.init(seed, 0u, id);
  c.npackets += 1;
  const int64_t cell = dust_emit_cells(g, src, s.rng, s.p);
  const LyaRecord r = l.records[cell];
  const double b = 1. / r.inv_b;
  const double r1 = sqrt(-log(s.rng.next()));
  const double f1 = 2. * M_PI * s.rng.next();
  const double r2 = sqrt(-log(s.rng.next()));
  const double f2 = 2. * M_PI * s.rng.next();
  const double w[3] = {r.v[0] + b * (r1 * cos(f1)), r.v[1] + b * (r1 * sin(f1)),
                       r.v[2] + b * (r2 * cos(f2))};
  s.q = dust_dot3(w, s.p.dir);
  s.albedo = 1.;
  s.nscatter = 0;
  lya_peel_views<CAMERA>(g, d, cam, l, s.p, 0, s.q, w, 1., 0., 0., dv, c, tr);
  if constexpr (FIELD)
    t.W = 1.;
  const double tau_max = lya_integrate<FIELD>(g, l.records, s.p.pos, s.p.dir,
                                              s.p.inv_dir, s.q, c.nsteps, t);
  s.forced = 1. - exp(-tau_max);
  const double tau = -log(1. - s.rng.next() * s.forced);
  s.alive = lya_interact<false>(g, l.records, s.p, s.q, tau, c.nsteps);
}

/* one event of a packet that is alive, and the walk to the next; the event's
 * cell counts the incoming weight as a collision (for dust: before the
 * albedo), the walk tallies the outgoing one */
template <int CAMERA, bool FIELD>
__device__ __forceinline__ void
lya_event(const GridDev &g, const DustDev &d, const DustCamera<CAMERA> &cam,
          const LyaDev &l, LyaState &s, DustDev &dv, LyaCountersDev &c,
          LyaTrace &tr, LyaTally<FIELD> &t) {
  const LyaRecord r = l.records[dust_cube_cell(g, s.p.pos)];
  const double k[3] = {s.p.dir[0], s.p.dir[1], s.p.dir[2]};
  double kH, x;
  const double kappa = lya_opacity(r, s.q, k, kH, x);
  if (s.rng.next() < kH / kappa) {
    if constexpr (FIELD)
      atomicAdd(t.rows + CMI_LYA_FIELD_ROW * dust_cube_cell(g, s.p.pos) +
                    LYA_FIELD_N_H,
                s.forced * s.albedo);
    const double b = 1. / r.inv_b;
    const double u_par = lya_sample_parallel(x, r.a, s.rng, c.nrejections);
    const double skip = (fabs(x) < l.x_crit) ? l.x_crit2 : 0.;
    const double rho = sqrt(skip - log(s.rng.next()));
    const double psi = 2. * M_PI * s.rng.next();
    const double u1 = rho * cos(psi), u2 = rho * sin(psi);
    /* e_1 = d k / d theta, e_2 = k x e_1 / sin theta ... from the photon's
     * angles {sin theta, cos theta, phi, sin phi, cos phi} */
    const double e1[3] = {s.p.par[1] * s.p.par[4], s.p.par[1] * s.p.par[3],
                          -s.p.par[0]};
    const double e2[3] = {-s.p.par[3], s.p.par[4], 0.};
    double w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      w[a] = r.v[a] + b * ((u_par * k[a] + u1 * e1[a]) + u2 * e2[a]);
    lya_peel_views<CAMERA>(g, d, cam, l, s.p, 1, s.q, w, s.forced * s.albedo,
                           u_par, x, dv, c, tr);
    lya_isotropic(s.rng, s.p);
    s.p.stokes[1] = 0.;
    s.p.stokes[2] = 0.;
    s.p.stokes[3] = 0.;
    s.q += dust_dot3(w, s.p.dir) - dust_dot3(w, k);
    c.nhydrogen += 1;
  } else {
    if constexpr (FIELD)
      atomicAdd(t.rows + CMI_LYA_FIELD_ROW * dust_cube_cell(g, s.p.pos) +
                    LYA_FIELD_N_D,
                s.forced * s.albedo);
    s.albedo *= d.albedo;
    lya_peel_views<CAMERA>(g, d, cam, l, s.p, 2, s.q, r.v, s.forced * s.albedo,
                           0., x, dv, c, tr);
    dust_scatter(d, s.rng, s.p);
    s.q += dust_dot3(r.v, s.p.dir) - dust_dot3(r.v, k);
    c.ndust += 1;
  }
  if (++s.nscatter >= l.max_scatter) {
    c.ncapped += 1;
    s.alive = false;
    return;
  }
  const double tau = -log(s.rng.next());
  if constexpr (FIELD)
    t.W = s.forced * s.albedo;
  s.alive = lya_interact<FIELD>(g, l.records, s.p, s.q, tau, c.nsteps, t);
}

__device__ __forceinline__ LyaTally<false> lya_tally_of() { return {}; }
__device__ __forceinline__ LyaTally<true> lya_tally_of(const LyaFieldDev &f) {
  return {f.rows, f.momentum_d, 0.};
}

/* packets [first, first + n); *next is 0 at the launch. FIELD is empty, or
 * LyaFieldDev for a launch that tallies the radiation field: the kernel
 * without it has the arguments it always had */
template <int CAMERA, typename... FIELD>
__global__ void __launch_bounds__(256)
    lya_shoot_kernel(GridDev g, DustDev d, CellSourceDev src,
                     DustCamera<CAMERA> cam, LyaDev l, uint32_t seed,
                     uint64_t first, uint64_t n, unsigned long long *next,
                     LyaCountersDev *counters, FIELD... field) {
  static_assert(sizeof...(FIELD) <= 1, "at most one field");
  constexpr bool TALLY = sizeof...(FIELD) == 1;
  LyaTally<TALLY> t = lya_tally_of(field...);
  LyaCountersDev c = {};
  LyaTrace tr = {nullptr, 0, 0};
  LyaState s;
  s.alive = false;
  DustDev dv;
  if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS)
    dv = d;
#ifndef CMI_LYA_EVENT_LOOP
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) {
    lya_begin<CAMERA, TALLY>(g, d, src, cam, l, seed, first + k, s, dv, c, tr,
                             t);
    while (s.alive)
      lya_event<CAMERA, TALLY>(g, d, cam, l, s, dv, c, tr, t);
  }
#else
  for (;;) {
    if (!s.alive) {
      const unsigned long long k = atomicAdd(next, 1ull);
      if (k >= n)
        break;
      lya_begin<CAMERA, TALLY>(g, d, src, cam, l, seed, first + k, s, dv, c,
                               tr, t);
    } else {
      lya_event<CAMERA, TALLY>(g, d, cam, l, s, dv, c, tr, t);
    }
  }
#endif
  /* the whole wave reaches the reduction */
  dust_count(&counters->nsteps, c.nsteps);
  dust_count(&counters->nhydrogen, c.nhydrogen);
  dust_count(&counters->ndust, c.ndust);
  dust_count(&counters->nrejections, c.nrejections);
  dust_count(&counters->natomics, c.natomics);
  dust_count(&counters->ncapped, c.ncapped);
  dust_count(&counters->npackets, c.npackets);
}

enum {
  LYA_PROBE_VOIGT = 0,
  LYA_PROBE_OPTICAL_DEPTH = 1,
  LYA_PROBE_SAMPLER = 2,
  LYA_PROBE_TRACE = 3
};
#define CMI_LYA_TRACE_HEADER 6

/* the parity probes of cmi_gpu_lya_probe (include/cmi_gpu.h gives the rows);
 * row k uses the stream of packet first + k */
template <int CAMERA>
__global__ void __launch_bounds__(64)
    lya_probe_kernel(GridDev g, DustDev d, CellSourceDev src,
                     DustCamera<CAMERA> cam, LyaDev l, int32_t kind,
                     uint32_t seed, uint64_t first, int64_t n, int32_t width,
                     const double *__restrict__ in, double *__restrict__ out,
                     int32_t max_events) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  double *o = out + k * width;
  if (kind == LYA_PROBE_VOIGT) {
    /* in: {a, x, kappa_0, kappa_d}; out: {H, kappa} */
    const double *r = in + 4 * k;
    o[0] = lya_voigt(r[0], r[1] * r[1]);
    o[1] = r[2] * o[0] + r[3];
  } else if (kind == LYA_PROBE_OPTICAL_DEPTH) {
    /* in: {pos[3], dir[3], q}; out: {tau, steps} */
    const double *r = in + 7 * k;
    const double inv[3] = {1. / r[3], 1. / r[4], 1. / r[5]};
    unsigned long long nsteps = 0;
    o[0] = lya_integrate<false>(g, l.records, r, r + 3, inv, r[6], nsteps);
    o[1] = (double)nsteps;
  } else if (kind == LYA_PROBE_SAMPLER) {
    /* in: {x, a}; out: {u_par, rejections} */
    PacketRng rng;
    rng.init(seed, 0u, first + k);
    unsigned long long nrej = 0;
    o[0] = lya_sample_parallel(in[2 * k], in[2 * k + 1], rng, nrej);
    o[1] = (double)nrej;
  } else if (kind == LYA_PROBE_TRACE) {
    /* out: {events, hydrogen, dust, steps, capped, rejections, rows} */
    LyaCountersDev c = {};
    LyaTrace tr = {o + CMI_LYA_TRACE_HEADER, max_events, 0};
    LyaState s;
    DustDev dv;
    if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS)
      dv = d;
    LyaTally<false> t;
    lya_begin<CAMERA, false>(g, d, src, cam, l, seed, first + k, s, dv, c, tr,
                             t);
    while (s.alive)
      lya_event<CAMERA, false>(g, d, cam, l, s, dv, c, tr, t);
    o[0] = tr.n;
    o[1] = (double)c.nhydrogen;
    o[2] = (double)c.ndust;
    o[3] = (double)c.nsteps;
    o[4] = (double)c.ncapped;
    o[5] = (double)c.nrejections;
  }
}

/* W m^-3 of Lyman alpha from recombinations per cell: f_alpha(T) alpha_B(T)
 * n_e n_p h nu_0 with alpha_B of Hui & Gnedin (1997) and f_alpha of Cantalupo
 * et al. (2008); n_e as free_free_pair has it; 0 without a temperature */
__global__ void __launch_bounds__(256)
    lya_emissivity_kernel(const double *__restrict__ number_density,
                          const double *__restrict__ temperature,
                          const double *__restrict__ x_H0,
                          const double *__restrict__ x_He0, double A_He,
                          int64_t ncell, double *__restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell)
    return;
  const double n = number_density[c], T = temperature[c];
  const double n_e = n * ((1. - x_H0[c]) + A_He * (1. - x_He0[c]));
  const double n_p = n * (1. - x_H0[c]);
  double j = 0.;
  if (T > 0.) {
    const double L = 315614. / T;
    const double alpha_B = 2.753e-14 * pow(L, 1.5) /
                           pow(1. + pow(L / 2.74, 0.407), 2.242) * 1.e-6;
    const double T4 = T / 1.e4;
    const double f_alpha = 0.686 - 0.106 * log10(T4) - 0.009 * pow(T4, -0.44);
    j = f_alpha * alpha_B * n_e * n_p *
        (CMI_PLANCK * CMI_LIGHTSPEED / CMI_LYA_LAMBDA0);
  }
  out[c] = j;
}

/* Wouthuysen-Field coupling (include/cmi_gpu.h, cmi_gpu_lya_spin_temperature,
 * has the formulas and their sources). The de-excitation rate coefficients in
 * m^3 s^-1: H-H of Kuhlen, Madau & Montgomery (2006), e-H of Liszt (2001) held
 * at its 1e4 K value above and at its 1 K value below */
#define CMI_LYA_KAPPA_HH 3.1e-17
__device__ __forceinline__ double lya_kappa_HH(double T) {
  return CMI_LYA_KAPPA_HH * pow(T, 0.357) * exp(-32. / T);
}
__device__ __forceinline__ double lya_kappa_eH(double T) {
  const double lT = log10(fmin(fmax(T, 1.), 1.e4));
  return 1.e-6 * pow(10., -9.607 + 0.5 * lT * exp(-pow(lT, 4.5) / 1800.));
}

struct LyaCouplingArgs {
  const double *rows; /* [ncell][8] */
  const LyaRecord *records;
  const double *number_density, *temperature, *x_H0, *x_He0; /* the cells */
  double A_He;
  double scale;       /* W per packet */
  double background;  /* T_gamma, K */
  double cell_volume; /* m^3 */
  int32_t collisions;
  int64_t ncell;
  double *P_alpha; /* [ncell] or null */
  double *T_s;     /* [ncell] */
};

/* the spin temperature of a cell from its scattering rate P, its kinetic
 * temperature and its collision rate C_10; the colour temperature of the
 * Lyman-alpha field is taken as T_k */
__device__ __forceinline__ double lya_spin_temperature(double P, double C_10,
                                                       double T_k,
                                                       double T_gamma) {
  if (!(T_k > 0.))
    return T_gamma;
  const double T_star = CMI_PLANCK * CMI_HI_FREQUENCY / CMI_BOLTZMANN;
  const double x_a = 4. * P * T_star / (27. * CMI_HI_EINSTEIN_A * T_gamma);
  const double x_c = (C_10 / CMI_HI_EINSTEIN_A) * (T_star / T_gamma);
  const double x = x_a + x_c;
  return (1. + x) / (1. / T_gamma + x / T_k);
}

/* one thread per cell: P_alpha = s S_H / (h nu_0 n_HI V), 0 where n_HI = 0,
 * and T_s */
__global__ void __launch_bounds__(256)
    lya_coupling_kernel(const LyaCouplingArgs a) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.ncell)
    return;
  const double n_HI = a.records[c].n_HI;
  const double S_H = a.rows[CMI_LYA_FIELD_ROW * c + LYA_FIELD_S_H];
  const double P =
      (n_HI > 0.) ? a.scale * S_H /
                        ((CMI_PLANCK * CMI_LIGHTSPEED / CMI_LYA_LAMBDA0) *
                         n_HI * a.cell_volume)
                  : 0.;
  const double T = a.temperature[c];
  double C_10 = 0.;
  if (a.collisions && T > 0.) {
    const double n = a.number_density[c];
    const double n_e = n * ((1. - a.x_H0[c]) + a.A_He * (1. - a.x_He0[c]));
    C_10 = n_HI * lya_kappa_HH(T) + n_e * lya_kappa_eH(T);
  }
  if (a.P_alpha)
    a.P_alpha[c] = P;
  a.T_s[c] = lya_spin_temperature(P, C_10, T, a.background);
}

#endif
