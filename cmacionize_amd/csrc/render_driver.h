/*
 * render_driver.h - the host side of the ray-traced renderers (included from
 * engine.hip): line images, line cubes, sky maps, sky cubes, the radio
 * continuum and the absorbing line cubes. A render call is
 *   - an arena that owns its device memory,
 *   - a source of per-cell records (the engine's cells or the caller's host
 *     fields), marched a batch at a time,
 *   - a camera: chunks of pixel rows for the parallel one, chunks of rays for
 *     the point observer,
 * and the entry points are argument checks and one call into these.
 *
 * The template kernels are first named here in the order line_image_march,
 * line_record, field_record, line_cube_march, sky_march, sky_cube_march,
 * continuum_march, continuum_sky_march, hi_record, hi_record_check,
 * field_absorbing_record, absorbing_cube_march, absorbing_sky_march, always
 * from a function that is no template itself: that order is the order of the
 * kernels in the code object (DESIGN_LOG.md 10 and 15).
 */
#ifndef CMI_RENDER_DRIVER_H
#define CMI_RENDER_DRIVER_H

extern "C++" {
namespace {
/* ------------------------------------------- a call's device memory -- */

/* owns the device buffers of one call and frees them however it ends */
struct RenderArena {
  static constexpr int MAX_BUFFERS = 16;
  void *owned[MAX_BUFFERS];
  int nowned = 0;
  /* an alloc failed for want of device memory: the callers that have a
   * message of their own for that (CMI_GPU_ENOMEM) ask here */
  bool out_of_memory = false;
  RenderArena() = default;
  RenderArena(const RenderArena &) = delete;
  RenderArena &operator=(const RenderArena &) = delete;
  ~RenderArena() {
    while (nowned)
      (void)hipFree(owned[--nowned]);
  }
  template <class T> int alloc(T *&p, size_t n) {
    if (nowned == MAX_BUFFERS)
      return fail(CMI_GPU_ESTATE, "a render call asked for more than %d "
                  "device buffers", MAX_BUFFERS);
    void *fresh = nullptr;
    const hipError_t err = hipMalloc(&fresh, sizeof(T) * n);
    if (err == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      out_of_memory = true;
    }
    HIP_TRY(err);
    owned[nowned++] = fresh;
    p = static_cast<T *>(fresh);
    return CMI_GPU_OK;
  }
  /* the caller has taken the buffers over (a setter that built its new state
   * aside and adopts it): nothing is freed */
  void release() { nowned = 0; }
  /* a device copy of the host array src[n] */
  int upload(double *&p, const double *src, size_t n) {
    CMI_TRY(alloc(p, n));
    HIP_TRY(hipMemcpy(p, src, sizeof(double) * n, hipMemcpyHostToDevice));
    return CMI_GPU_OK;
  }
};

/* ------------------------------------------------- argument checks -- */

int check_lines(const char *what, int32_t nlines, const int32_t *lines,
                bool needs_profile) {
  if (nlines < 1 || nlines > CMI_NEMISSIONLINE)
    return fail(CMI_GPU_EINVAL, "%s: %d lines asked for, there are %d", what,
                (int)nlines, CMI_NEMISSIONLINE);
  for (int32_t l = 0; l < nlines; ++l) {
    if (lines[l] < 0 || lines[l] >= CMI_NEMISSIONLINE)
      return fail(CMI_GPU_EINVAL, "%s: no emission line %d", what,
                  (int)lines[l]);
    if (needs_profile && cmi_emission_atomic_weight[lines[l]] == 0.)
      return fail(CMI_GPU_EINVAL, "%s: entry %d is not the line of one ion: "
                  "it has no line profile", what, (int)lines[l]);
  }
  return CMI_GPU_OK;
}

int check_field_count(const char *what, int32_t nfields) {
  if (nfields < 1 || nfields > 1024)
    return fail(CMI_GPU_EINVAL, "%s: between 1 and 1024 fields (%d asked for)",
                what, (int)nfields);
  return CMI_GPU_OK;
}

int check_dust_cross_section(const char *what, double dust_cross_section) {
  if (!(dust_cross_section >= 0.) || !std::isfinite(dust_cross_section))
    return fail(CMI_GPU_EINVAL, "%s: the dust cross section must be >= 0",
                what);
  return CMI_GPU_OK;
}

int check_sigma_turb(const char *what, double sigma_turb) {
  if (!(sigma_turb >= 0.) || !std::isfinite(sigma_turb))
    return fail(CMI_GPU_EINVAL, "%s: the turbulent velocity dispersion must "
                "be >= 0 and finite", what);
  return CMI_GPU_OK;
}

/* widths[nfields][ncell] (host) */
int check_widths(const char *what, const double *widths, size_t ncell,
                 int32_t nfields) {
  for (size_t i = 0; i < ncell * (size_t)nfields; ++i)
    if (!(widths[i] >= 0.) || !std::isfinite(widths[i]))
      return fail(CMI_GPU_EINVAL, "%s: the width of field %lld in cell %lld "
                  "is negative or not finite", what, (long long)(i / ncell),
                  (long long)(i % ncell));
  return CMI_GPU_OK;
}

int check_have_cells(const cmi_gpu_engine *e, const char *what) {
  if (!e->have_cells)
    return fail(CMI_GPU_ESTATE, "%s: cell data must be set first", what);
  return CMI_GPU_OK;
}

/* n image coordinates xy[n][2] (host) of a probe */
int check_image_coordinates(const char *what, int64_t n, const double *xy) {
  for (int64_t k = 0; k < 2 * n; ++k)
    if (!std::isfinite(xy[k]))
      return fail(CMI_GPU_EINVAL, "%s: image coordinate %lld of ray %lld is "
                  "not finite", what, (long long)(k % 2), (long long)(k / 2));
  return CMI_GPU_OK;
}

int line_image_view(const cmi_gpu_engine *e, const char *what, double theta,
                    double phi, LineViewDev &v) {
  const GridDev &g = e->grid;
  if (g.decomposed)
    return fail(CMI_GPU_ESTATE, "%s: not available on a block of a decomposed "
                "grid (an image of one block is not an image)", what);
  if (g.periodic[0] || g.periodic[1] || g.periodic[2])
    return fail(CMI_GPU_EINVAL, "%s: periodic boxes are not supported (a line "
                "of sight through a periodic box has no end)", what);
  if (!std::isfinite(theta) || !std::isfinite(phi))
    return fail(CMI_GPU_EINVAL, "%s: view angles must be finite", what);
  const double st = std::sin(theta), ct = std::cos(theta);
  const double sp = std::sin(phi), cp = std::cos(phi);
  v.n[0] = st * cp;
  v.n[1] = st * sp;
  v.n[2] = ct;
  v.ex[0] = -sp;
  v.ex[1] = cp;
  v.ex[2] = 0.;
  v.ey[0] = -ct * cp;
  v.ey[1] = -ct * sp;
  v.ey[2] = st;
  for (int a = 0; a < 3; ++a)
    v.inv_n[a] = 1. / v.n[a];
  v.nx = v.ny = v.s = 1;
  v.pad = 0;
  v.img_anchor[0] = v.img_anchor[1] = 0.;
  v.img_sides[0] = v.img_sides[1] = 1.;
  return CMI_GPU_OK;
}

int line_image_geometry(const cmi_gpu_engine *e, const char *what,
                        double theta, double phi, int32_t nx, int32_t ny,
                        const double *anchor, const double *sides,
                        int32_t supersample, LineViewDev &v) {
  if (!anchor || !sides)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  if (nx <= 0 || ny <= 0 || (int64_t)nx * ny > (1ll << 28))
    return fail(CMI_GPU_EINVAL, "%s: the image must have between 1 and 2^28 "
                "pixels (%d x %d asked for)", what, (int)nx, (int)ny);
  if (supersample < 1 || supersample > CMI_LINE_IMAGE_MAX_SUPERSAMPLE)
    return fail(CMI_GPU_EINVAL, "%s: supersampling must be 1..%d (%d asked "
                "for)", what, CMI_LINE_IMAGE_MAX_SUPERSAMPLE, (int)supersample);
  /* the sample grid is indexed with 32-bit integers */
  if ((int64_t)nx * supersample > (1ll << 30) ||
      (int64_t)ny * supersample > (1ll << 30))
    return fail(CMI_GPU_EINVAL, "%s: %d x %d pixels at supersampling %d: more "
                "than 2^30 samples along an axis", what, (int)nx, (int)ny,
                (int)supersample);
  if (!(sides[0] > 0.) || !(sides[1] > 0.) || !std::isfinite(sides[0]) ||
      !std::isfinite(sides[1]) || !std::isfinite(anchor[0]) ||
      !std::isfinite(anchor[1]))
    return fail(CMI_GPU_EINVAL, "%s: the image sides must be positive", what);
  CMI_TRY(line_image_view(e, what, theta, phi, v));
  v.nx = nx;
  v.ny = ny;
  v.s = supersample;
  for (int a = 0; a < 2; ++a) {
    v.img_anchor[a] = anchor[a];
    v.img_sides[a] = sides[a];
  }
  return CMI_GPU_OK;
}

/* the velocity axis of a cube call */
struct LineCubeAxis {
  int32_t nchan;
  double vmin, dv;
};

int line_cube_axis(const char *what, int32_t nplanes, int32_t nx, int32_t ny,
                   int32_t nchan, double vmin, double vmax,
                   LineCubeAxis &axis) {
  if (nchan < 1)
    return fail(CMI_GPU_EINVAL, "%s: at least one velocity channel (%d asked "
                "for)", what, (int)nchan);
  if (!std::isfinite(vmin) || !std::isfinite(vmax) || !(vmax > vmin) ||
      !std::isfinite(vmax - vmin))
    return fail(CMI_GPU_EINVAL, "%s: the velocity range must be finite with "
                "vmax > vmin", what);
  /* (nx ny <= 2^28 has been checked, so the products below cannot overflow) */
  if ((int64_t)nplanes * nchan > (1ll << 28) ||
      (int64_t)nplanes * nchan * ((int64_t)nx * ny) > (1ll << 28))
    return fail(CMI_GPU_EINVAL, "%s: %d x %d channels of %d x %d pixels: a "
                "cube has at most 2^28 values", what, (int)nplanes, (int)nchan,
                (int)nx, (int)ny);
  axis.nchan = nchan;
  axis.vmin = vmin;
  axis.dv = (vmax - vmin) / nchan;
  return CMI_GPU_OK;
}

/* what every sky call asks of the engine and of its rays before a launch */
int sky_check(const cmi_gpu_engine *e, const char *what, const double *origin,
              int64_t nrays, int64_t max_rays, const double *directions) {
  const GridDev &g = e->grid;
  if (g.decomposed)
    return fail(CMI_GPU_ESTATE, "%s: not available on a block of a decomposed "
                "grid (the sky of one block is not a sky)", what);
  if (g.periodic[0] || g.periodic[1] || g.periodic[2])
    return fail(CMI_GPU_EINVAL, "%s: periodic boxes are not supported (a line "
                "of sight through a periodic box has no end)", what);
  if (nrays <= 0 || nrays > max_rays)
    return fail(CMI_GPU_EINVAL, "%s: between 1 and %lld rays (%lld asked for)",
                what, (long long)max_rays, (long long)nrays);
  if (!origin || !directions)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(origin[a]))
      return fail(CMI_GPU_EINVAL, "%s: component %d of the origin is not "
                  "finite", what, a);
  for (int64_t r = 0; r < nrays; ++r) {
    const double *d = directions + 3 * r;
    if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2]))
      return fail(CMI_GPU_EINVAL, "%s: the direction of ray %lld is not "
                  "finite", what, (long long)r);
    const double norm2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!(std::fabs(norm2 - 1.) <= 1.e-9))
      return fail(CMI_GPU_EINVAL, "%s: the direction of ray %lld is not a "
                  "unit vector (|d|^2 = %.17g)", what, (long long)r, norm2);
  }
  return CMI_GPU_OK;
}

/* the size, the velocity axis and the observer's velocity of a sky cube call
 * (sky_check has bounded nrays) */
int sky_cube_check(const char *what, int32_t nplanes, int64_t nrays,
                   int32_t nchan, double vmin, double vmax,
                   const double *observer_velocity, LineCubeAxis &axis,
                   double v_obs[3]) {
  if (nchan >= 1 &&
      ((int64_t)nplanes * nchan > (1ll << 28) ||
       (int64_t)nplanes * nchan * nrays > (1ll << 28)))
    return fail(CMI_GPU_EINVAL, "%s: %d x %d channels of %lld rays: a cube has "
                "at most 2^28 values", what, (int)nplanes, (int)nchan,
                (long long)nrays);
  CMI_TRY(line_cube_axis(what, nplanes, 1, 1, nchan, vmin, vmax, axis));
  for (int a = 0; a < 3; ++a) {
    v_obs[a] = observer_velocity ? observer_velocity[a] : 0.;
    if (!std::isfinite(v_obs[a]))
      return fail(CMI_GPU_EINVAL, "%s: component %d of the observer's velocity "
                  "is not finite", what, a);
  }
  return CMI_GPU_OK;
}

/* bad = how many of the n values of a device array are not finite */
int count_not_finite(cmi_gpu_engine *e, const double *values, int64_t n,
                     unsigned int &bad) {
  RenderArena arena;
  unsigned int *ninvalid = nullptr;
  CMI_TRY(arena.alloc(ninvalid, 1));
  bad = 0;
  HIP_TRY(hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream));
  cell_velocity_check_kernel<<<grid_blocks(e, n, 8), 256, 0, e->stream>>>(
      values, n, ninvalid);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

/* refuses a device array of n velocities of which one is not finite */
int line_cube_check_velocities(cmi_gpu_engine *e, const char *what,
                               const double *velocity, int64_t n) {
  unsigned int bad = 0;
  CMI_TRY(count_not_finite(e, velocity, n, bad));
  if (bad)
    return fail(CMI_GPU_EINVAL, "%s: %u velocity component(s) are not finite",
                what, bad);
  return CMI_GPU_OK;
}

/* -------------------------------------------------- the two cameras -- */

/* The parallel camera: an image of planes [nplanes][nx * ny] on the device,
 * marched in chunks of pixel rows of at most launch_samples sample rays. With
 * supersampling a chunk is marched into the sample buffer and reduced into
 * the image; without, straight into the image. */
struct ParallelCamera {
  cmi_gpu_engine *e = nullptr;
  LineViewDev v;
  int64_t npixel = 0, NY = 0, rows = 0, chunk_samples = 0;
  double *samples = nullptr, *image = nullptr;
  int64_t ix0 = 0, ix1 = 0; /* the pixel rows of the chunk being marched */

  /* sample_planes: planes one chunk's launches write before they are reduced;
   * image_planes: planes of the image */
  int begin(cmi_gpu_engine *engine, const LineViewDev &view,
            int64_t launch_samples, int sample_planes, size_t image_planes,
            RenderArena &arena) {
    e = engine;
    v = view;
    npixel = (int64_t)v.nx * v.ny;
    NY = (int64_t)v.ny * v.s;
    rows = std::max<int64_t>(
        1, std::min<int64_t>(v.nx, launch_samples / (NY * v.s)));
    chunk_samples = rows * v.s * NY;
    CMI_TRY(arena.alloc(image, (size_t)npixel * image_planes));
    if (sampled())
      CMI_TRY(arena.alloc(samples, (size_t)chunk_samples * sample_planes));
    return CMI_GPU_OK;
  }
  bool sampled() const { return v.s > 1; }

  /* enqueue() puts the march launch(es) of the chunk on the stream */
  template <class F> int march(F &&enqueue) {
    for (ix0 = 0; ix0 < v.nx; ix0 += rows) {
      ix1 = std::min<int64_t>(v.nx, ix0 + rows);
      CMI_TRY(enqueue());
    }
    return CMI_GPU_OK;
  }
  /* of the chunk: its sample columns, its wave tiles, where a launch writes
   * what ends as image plane p when it is the launch's first plane, and the
   * distance between two planes there */
  int32_t sx0() const { return (int32_t)(ix0 * v.s); }
  int32_t sx1() const { return (int32_t)(ix1 * v.s); }
  unsigned tiles() const { return tile_workgroups(sx1() - sx0(), NY); }
  double *out(int64_t p) const {
    return sampled() ? samples : image + p * npixel + ix0 * v.ny;
  }
  int64_t plane_stride() const { return sampled() ? chunk_samples : npixel; }
  /* sample planes [sample_plane, + nplanes) of the chunk into the image
   * planes from image_plane on (nothing to do without supersampling) */
  int reduce(int64_t sample_plane, int nplanes, int64_t image_plane) const {
    if (!sampled())
      return CMI_GPU_OK;
    const int64_t work = (ix1 - ix0) * v.ny * nplanes;
    line_image_reduce_kernel<<<(unsigned)((work + 255) / 256), 256, 0,
                               e->stream>>>(
        samples + sample_plane * chunk_samples, chunk_samples, nplanes,
        (int32_t)ix0, (int32_t)ix1, v.ny, v.s, npixel,
        image + image_plane * npixel);
    HIP_TRY(hipGetLastError());
    return CMI_GPU_OK;
  }
  /* waits for the marches and copies the first nplanes planes to the host */
  int download(double *host, size_t nplanes) const {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(host, image, sizeof(double) * (size_t)npixel * nplanes,
                      hipMemcpyDeviceToHost));
    return CMI_GPU_OK;
  }
};

/* The point observer: rays from origin along directions[nrays][3] (host),
 * marched in chunks of at most launch_rays rays: directions up, march,
 * results down. */
struct PointCamera {
  cmi_gpu_engine *e = nullptr;
  const double *origin = nullptr, *host_directions = nullptr;
  int64_t nrays = 0, chunk = 0;
  double *directions = nullptr, *out = nullptr; /* device, of one chunk */
  /* a call that one chunk holds comes down in one copy, not plane by plane
   * (the sky cubes: many short planes) */
  bool one_copy = false;

  /* out_planes: planes [chunk] one chunk's launches write */
  int begin(cmi_gpu_engine *engine, const double *origin_, int64_t nrays_,
            const double *directions_, int64_t launch_rays, size_t out_planes,
            RenderArena &arena) {
    e = engine;
    origin = origin_;
    host_directions = directions_;
    nrays = nrays_;
    chunk = std::max<int64_t>(1, std::min<int64_t>(nrays, launch_rays));
    CMI_TRY(arena.alloc(directions, 3 * (size_t)chunk));
    CMI_TRY(arena.alloc(out, (size_t)chunk * out_planes));
    return CMI_GPU_OK;
  }
  /* enqueue(n) puts the march launch(es) of a chunk of n rays on the stream:
   * plane p of ray r to out[p * chunk + r]. The planes [nplanes][nrays] end
   * in host_out. */
  template <class F> int march(size_t nplanes, double *host_out, F &&enqueue) {
    for (int64_t r0 = 0; r0 < nrays; r0 += chunk) {
      const int64_t n = std::min<int64_t>(chunk, nrays - r0);
      HIP_TRY(hipMemcpy(directions, host_directions + 3 * r0,
                        sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
      CMI_TRY(enqueue(n));
      HIP_TRY(hipStreamSynchronize(e->stream));
      if (one_copy && n == nrays) {
        /* one chunk holds the call: the planes are contiguous on both sides */
        HIP_TRY(hipMemcpy(host_out, out, sizeof(double) * nplanes * (size_t)n,
                          hipMemcpyDeviceToHost));
      } else {
        for (size_t p = 0; p < nplanes; ++p)
          HIP_TRY(hipMemcpy(host_out + p * (size_t)nrays + r0,
                            out + p * (size_t)chunk,
                            sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
      }
    }
    return CMI_GPU_OK;
  }
};

/* ------------------------------------------------ the plain records -- */

/* f(std::integral_constant<int, ND>) for the record of nd doubles: 2, 4, 6
 * or 8 (line_image_record_doubles) */
template <class F> void line_image_for_record(int nd, F &&f) {
  switch (nd) {
  case 2: f(std::integral_constant<int, 2>()); break;
  case 4: f(std::integral_constant<int, 4>()); break;
  case 6: f(std::integral_constant<int, 6>()); break;
  default: f(std::integral_constant<int, 8>()); break;
  }
}

template <int ND>
void line_image_launch_march(cmi_gpu_engine *e, const LineMarchArgs &a,
                             unsigned tiles) {
  line_image_march_kernel<ND><<<tiles, 256, 0, e->stream>>>(a);
}

/* doubles of the record of a batch of nl lines: {k, s[nl]} padded to 16 B */
inline int line_image_record_doubles(int nl) { return (nl + 2) & ~1; }

/* image planes [nl][nx * ny] of the records [ncell][nd] */
int line_image_march(ParallelCamera &cam, const double *records, int nl) {
  const int nd = line_image_record_doubles(nl);
  return cam.march([&]() -> int {
    LineMarchArgs a;
    a.grid = cam.e->grid;
    a.view = cam.v;
    a.records = records;
    a.sx0 = cam.sx0();
    a.sx1 = cam.sx1();
    a.nlines = nl;
    a.out = cam.out(0);
    a.line_stride = cam.plane_stride();
    line_image_for_record(nd, [&](auto width) {
      line_image_launch_march<decltype(width)::value>(cam.e, a, cam.tiles());
    });
    HIP_TRY(hipGetLastError());
    return cam.reduce(0, nl, 0);
  });
}

/* --------------------------------------------- where records come from -- */

/* the three layouts of a cell's record for a batch of nl lines or fields */
enum RecordLayout {
  RECORDS_PLAIN,   /* {k, s[nl]} padded to 16 B */
  RECORDS_CUBE,    /* 2 + 2 nl doubles; frame = the direction to the observer */
  RECORDS_SKY_CUBE /* 4 + 2 nl doubles; frame = the observer's velocity */
};

/* A source of records: count emission lines of the engine's cells (lines
 * set), or the caller's host fields[count][ncell] with optional
 * widths[count][ncell] (the cube layouts), extinction[ncell] and
 * velocity[3][ncell]. */
struct RecordSource {
  RecordLayout layout = RECORDS_PLAIN;
  int32_t count = 0;
  const int32_t *lines = nullptr;
  double dust_cross_section = 0., sigma_turb = 0.;
  const double *fields = nullptr, *widths = nullptr, *extinction = nullptr,
               *velocity = nullptr;
  double frame[3] = {0., 0., 0.};
  /* device */
  double *records = nullptr, *dfields = nullptr, *dwidths = nullptr,
         *dextinction = nullptr, *dvelocity = nullptr;

  int batch() const {
    return layout == RECORDS_SKY_CUBE ? CMI_SKY_CUBE_BATCH
                                      : CMI_LINE_IMAGE_BATCH;
  }
  int doubles(int nl) const {
    return layout == RECORDS_PLAIN  ? line_image_record_doubles(nl)
           : layout == RECORDS_CUBE ? 2 + 2 * nl
                                    : 4 + 2 * nl;
  }
  void set_frame(const double *f) {
    for (int a = 0; a < 3; ++a)
      frame[a] = f[a];
  }
  /* allocates, and uploads what is uploaded once */
  int begin(cmi_gpu_engine *e, const char *what, RenderArena &arena);
  /* the records of the batch [first, first + nl) onto the stream */
  int records_of(cmi_gpu_engine *e, int32_t first, int nl);
};

int RecordSource::begin(cmi_gpu_engine *e, const char *what,
                        RenderArena &arena) {
  const size_t ncell = (size_t)e->ncell;
  if (lines) {
    dvelocity = e->cell_velocities;
  } else if (velocity) {
    CMI_TRY(arena.upload(dvelocity, velocity, 3 * ncell));
    CMI_TRY(line_cube_check_velocities(e, what, dvelocity, 3 * (int64_t)ncell));
  }
  const int nb = std::min<int>(count, batch());
  CMI_TRY(arena.alloc(records, ncell * doubles(nb)));
  if (lines)
    return CMI_GPU_OK;
  CMI_TRY(arena.alloc(dfields, ncell * nb));
  if (widths)
    CMI_TRY(arena.alloc(dwidths, ncell * nb));
  if (extinction)
    CMI_TRY(arena.upload(dextinction, extinction, ncell));
  return CMI_GPU_OK;
}

/* the arguments of the two cube record kernels, which differ in the name of
 * the frame vector */
template <class Args>
void fill_cube_record_args(const cmi_gpu_engine *e, const CellsDev &cells,
                           const RecordSource &s, int32_t first, int nl,
                           Args &r, double *frame) {
  constexpr int BATCH = sizeof r.lines / sizeof r.lines[0];
  r.model = e->model;
  r.cells = cells;
  r.ncell = e->ncell;
  r.nlines = nl;
  for (int l = 0; l < BATCH; ++l) {
    r.lines[l] = l < nl ? s.lines[first + l] : 0;
    r.weight[l] = l < nl ? cmi_emission_atomic_weight[s.lines[first + l]] : 1.;
  }
  r.dust_cross_section = s.dust_cross_section;
  r.sigma_turb = s.sigma_turb;
  for (int a = 0; a < 3; ++a)
    frame[a] = s.frame[a];
  r.velocity = s.dvelocity;
  r.records = s.records;
}

int RecordSource::records_of(cmi_gpu_engine *e, int32_t first, int nl) {
  if (lines) {
    const int blocks = grid_blocks(e, e->ncell, 8);
    CellsDev *cells;
    CMI_TRY(cells_settled(e, cells));
    if (layout == RECORDS_PLAIN) {
      LineRecordArgs r;
      r.model = e->model;
      r.cells = *cells;
      r.ncell = e->ncell;
      r.nlines = nl;
      for (int l = 0; l < CMI_LINE_IMAGE_BATCH; ++l)
        r.lines[l] = l < nl ? lines[first + l] : 0;
      r.dust_cross_section = dust_cross_section;
      r.records = records;
      line_image_for_record(doubles(nl), [&](auto width) {
        line_record_kernel<decltype(width)::value>
            <<<blocks, CMI_BLOCK, 0, e->stream>>>(r);
      });
    } else if (layout == RECORDS_CUBE) {
      LineCubeRecordArgs r;
      fill_cube_record_args(e, *cells, *this, first, nl, r, r.n);
      line_cube_record_kernel<<<blocks, CMI_BLOCK, 0, e->stream>>>(r);
    } else {
      SkyCubeRecordArgs r;
      fill_cube_record_args(e, *cells, *this, first, nl, r, r.v_obs);
      sky_cube_record_kernel<<<blocks, CMI_BLOCK, 0, e->stream>>>(r);
    }
  } else {
    const size_t ncell = (size_t)e->ncell;
    HIP_TRY(hipMemcpy(dfields, fields + (size_t)first * ncell,
                      sizeof(double) * ncell * nl, hipMemcpyHostToDevice));
    if (widths)
      HIP_TRY(hipMemcpy(dwidths, widths + (size_t)first * ncell,
                        sizeof(double) * ncell * nl, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((e->ncell + 255) / 256);
    if (layout == RECORDS_PLAIN)
      line_image_for_record(doubles(nl), [&](auto width) {
        field_record_kernel<decltype(width)::value>
            <<<blocks, 256, 0, e->stream>>>(dfields, dextinction, e->ncell, nl,
                                            records);
      });
    else if (layout == RECORDS_CUBE)
      field_cube_record_kernel<<<blocks, 256, 0, e->stream>>>(
          dfields, dwidths, dextinction, dvelocity, frame[0], frame[1],
          frame[2], e->ncell, nl, records);
    else
      field_sky_cube_record_kernel<<<blocks, 256, 0, e->stream>>>(
          dfields, dwidths, dextinction, dvelocity, frame[0], frame[1],
          frame[2], e->ncell, nl, records);
  }
  HIP_TRY(hipGetLastError());
  return CMI_GPU_OK;
}

/* The batch loop of every renderer: the records of a batch, then
 * camera(first, n), which marches them and brings the result down. */
template <class Source, class Camera>
int render_batches(cmi_gpu_engine *e, Source &src, Camera &&camera) {
  const int32_t batch = src.batch();
  for (int32_t first = 0; first < src.count; first += batch) {
    const int n = std::min<int32_t>(src.count - first, batch);
    CMI_TRY(src.records_of(e, first, n));
    CMI_TRY(camera(first, n));
  }
  return CMI_GPU_OK;
}

/* ------------------------------------- line and field renderers -- */

/* images[count][nx * ny] (host) */
int render_images(cmi_gpu_engine *e, const char *what, RecordSource &src,
                  const LineViewDev &v, double *images) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  ParallelCamera cam;
  CMI_TRY(src.begin(e, what, arena));
  CMI_TRY(cam.begin(e, v, CMI_LINE_IMAGE_LAUNCH_SAMPLES, CMI_LINE_IMAGE_BATCH,
                    std::min<int>(src.count, src.batch()), arena));
  return render_batches(e, src, [&](int32_t first, int nl) -> int {
    CMI_TRY(line_image_march(cam, src.records, nl));
    return cam.download(images + (size_t)first * cam.npixel, nl);
  });
}

/* the cube planes [nl][nchan][nx * ny] of the records [ncell][2 + 2 nl]: per
 * chunk of pixel rows and per block of CB channels one march launch for the
 * nl lines */
int line_cube_march(ParallelCamera &cam, const double *records, int nl,
                    const LineCubeAxis &axis) {
  constexpr int CB = CMI_LINE_CUBE_CB;
  return cam.march([&]() -> int {
    for (int32_t c0 = 0; c0 < axis.nchan; c0 += CB) {
      LineCubeMarchArgs a;
      a.grid = cam.e->grid;
      a.view = cam.v;
      a.records = records;
      a.nd = 2 + 2 * nl;
      a.sx0 = cam.sx0();
      a.sx1 = cam.sx1();
      a.c0 = c0;
      a.nc = std::min<int32_t>(CB, axis.nchan - c0);
      a.vmin = axis.vmin;
      a.dv = axis.dv;
      a.out = cam.out(c0);
      a.channel_stride = cam.plane_stride();
      /* (the sample buffer holds CB channels of a line, the cube all) */
      a.line_stride = a.channel_stride * (cam.sampled() ? CB : axis.nchan);
      line_cube_march_kernel<CB>
          <<<dim3(cam.tiles(), (unsigned)nl), 256, 0, cam.e->stream>>>(a);
      HIP_TRY(hipGetLastError());
      /* the images' reduction, a line's channels in the place of lines */
      for (int l = 0; l < nl; ++l)
        CMI_TRY(cam.reduce((int64_t)l * CB, a.nc,
                           (int64_t)l * axis.nchan + c0));
    }
    return CMI_GPU_OK;
  });
}

/* cube[count][nchan][nx * ny] (host) */
int render_cube(cmi_gpu_engine *e, const char *what, RecordSource &src,
                const LineViewDev &v, const LineCubeAxis &axis, double *cube) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  ParallelCamera cam;
  CMI_TRY(src.begin(e, what, arena));
  /* (the sample buffer holds CB channels of a chunk's rows) */
  CMI_TRY(cam.begin(e, v, CMI_LINE_IMAGE_LAUNCH_SAMPLES / CMI_LINE_CUBE_CB,
                    CMI_LINE_CUBE_CB * CMI_LINE_IMAGE_BATCH,
                    (size_t)axis.nchan * std::min<int>(src.count, src.batch()),
                    arena));
  const size_t nvalue = (size_t)cam.npixel * axis.nchan; /* of one line */
  return render_batches(e, src, [&](int32_t first, int nl) -> int {
    CMI_TRY(line_cube_march(cam, src.records, nl, axis));
    return cam.download(cube + (size_t)first * nvalue,
                        (size_t)nl * axis.nchan);
  });
}

/* out[count][nrays] (host) */
int render_sky(cmi_gpu_engine *e, const char *what, RecordSource &src,
               const double *origin, int64_t nrays, const double *directions,
               double *out) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  PointCamera cam;
  CMI_TRY(src.begin(e, what, arena));
  CMI_TRY(cam.begin(e, origin, nrays, directions, CMI_SKY_LAUNCH_RAYS,
                    CMI_LINE_IMAGE_BATCH, arena));
  return render_batches(e, src, [&](int32_t first, int nl) -> int {
    const int nd = src.doubles(nl);
    return cam.march(nl, out + (size_t)first * nrays, [&](int64_t n) -> int {
      SkyMarchArgs a;
      a.grid = e->grid;
      for (int k = 0; k < 3; ++k)
        a.origin[k] = origin[k];
      a.directions = cam.directions;
      a.records = src.records;
      a.nrays = n;
      a.nlines = nl;
      a.pad = 0;
      a.line_stride = cam.chunk;
      a.out = cam.out;
      line_image_for_record(nd, [&](auto width) {
        sky_march_kernel<decltype(width)::value>
            <<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(a);
      });
      HIP_TRY(hipGetLastError());
      return CMI_GPU_OK;
    });
  });
}

/* values of one march's result buffer (bounds the rays per launch) */
constexpr int64_t CMI_SKY_CUBE_LAUNCH_VALUES = 1ll << 26;

/* out[count][nchan][nrays] (host): per chunk of rays and per block of CB
 * channels one march launch for the nl lines of a batch */
int render_sky_cube(cmi_gpu_engine *e, const char *what, RecordSource &src,
                    const double *origin, int64_t nrays,
                    const double *directions, const LineCubeAxis &axis,
                    double *out) {
  constexpr int CB = CMI_SKY_CUBE_CB;
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  PointCamera cam;
  CMI_TRY(src.begin(e, what, arena));
  const int64_t nb = std::min<int>(src.count, src.batch());
  CMI_TRY(cam.begin(e, origin, nrays, directions,
                    std::min<int64_t>(CMI_SKY_LAUNCH_RAYS,
                                      CMI_SKY_CUBE_LAUNCH_VALUES /
                                          (nb * axis.nchan)),
                    (size_t)(nb * axis.nchan), arena));
  cam.one_copy = true;
  return render_batches(e, src, [&](int32_t first, int nl) -> int {
    return cam.march(
        (size_t)nl * axis.nchan,
        out + (size_t)first * axis.nchan * (size_t)nrays,
        [&](int64_t n) -> int {
          for (int32_t c0 = 0; c0 < axis.nchan; c0 += CB) {
            SkyCubeMarchArgs a;
            a.grid = e->grid;
            for (int k = 0; k < 3; ++k)
              a.origin[k] = origin[k];
            a.directions = cam.directions;
            a.records = src.records;
            a.nrays = n;
            a.nd = 4 + 2 * nl;
            a.c0 = c0;
            a.nc = std::min<int32_t>(CB, axis.nchan - c0);
            a.pad = 0;
            a.vmin = axis.vmin;
            a.dv = axis.dv;
            a.line_stride = (int64_t)axis.nchan * cam.chunk;
            a.channel_stride = cam.chunk;
            a.out = cam.out;
            sky_cube_march_kernel<CB>
                <<<dim3((unsigned)((n + 255) / 256), (unsigned)nl), 256, 0,
                   e->stream>>>(a);
            HIP_TRY(hipGetLastError());
          }
          return CMI_GPU_OK;
        });
  });
}

/* ---------------------------------------------------- the map calls -- */

/* rows of a 3 x 3 frame orthonormal to 1e-9? */
bool sky_frame_is_orthonormal(const double *frame) {
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      double dot = 0.;
      for (int a = 0; a < 3; ++a)
        dot += frame[3 * i + a] * frame[3 * j + a];
      if (!(std::fabs(dot - (i == j ? 1. : 0.)) <= 1.e-9))
        return false;
    }
  return true;
}

int sky_map_check(const char *what, const double *frame, double lon_min,
                  double lon_max, double lat_min, double lat_max,
                  int32_t nlon, int32_t nlat) {
  if (!frame)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  if (nlon <= 0 || nlat <= 0 || (int64_t)nlon * nlat > (1ll << 28))
    return fail(CMI_GPU_EINVAL, "%s: the map must have between 1 and 2^28 "
                "pixels (%d x %d asked for)", what, (int)nlon, (int)nlat);
  if (!std::isfinite(lon_min) || !std::isfinite(lon_max) ||
      !(lon_min < lon_max))
    return fail(CMI_GPU_EINVAL, "%s: the longitude range must be finite and "
                "increasing", what);
  if (!(lat_min < lat_max) || !(lat_min >= -0.5 * M_PI) ||
      !(lat_max <= 0.5 * M_PI))
    return fail(CMI_GPU_EINVAL, "%s: the latitude range must be increasing "
                "and within [-pi / 2, pi / 2]", what);
  if (!sky_frame_is_orthonormal(frame))
    return fail(CMI_GPU_EINVAL, "%s: the frame is not orthonormal to 1e-9",
                what);
  return CMI_GPU_OK;
}

/* direction of the centre of pixel (i, j) */
void sky_map_direction(const double *frame, double lon_min, double lon_max,
                       double lat_min, double lat_max, int32_t nlon,
                       int32_t nlat, int32_t i, int32_t j, double *d) {
  const double l = lon_min + (lon_max - lon_min) * (i + 0.5) / nlon;
  const double b = lat_min + (lat_max - lat_min) * (j + 0.5) / nlat;
  const double cb = std::cos(b), sb = std::sin(b);
  const double c1 = cb * std::cos(l), c2 = cb * std::sin(l);
  for (int a = 0; a < 3; ++a)
    d[a] = c1 * frame[a] + c2 * frame[3 + a] + sb * frame[6 + a];
}

/* The rays of a map call in 8 x 8 tiles of the map, so that a wave's 64 rays
 * are neighbours on the sky; pixel[k] is the pixel of ray k. rays receives
 * the planes [nplanes][npixel] in ray order, scatter() puts them in pixel
 * order. */
struct SkyMapRays {
  size_t npixel = 0, nplanes = 0;
  std::vector<int64_t> pixel;
  std::vector<double> directions, rays;

  int begin(const char *what, const double *frame, double lon_min,
            double lon_max, double lat_min, double lat_max, int32_t nlon,
            int32_t nlat, size_t nplanes_) {
    npixel = (size_t)nlon * nlat;
    nplanes = nplanes_;
    try {
      pixel.reserve(npixel);
      directions.resize(3 * npixel);
      rays.resize(nplanes * npixel);
    } catch (const std::bad_alloc &) {
      return fail(CMI_GPU_ENOMEM, "%s: out of host memory", what);
    }
    for (int32_t i0 = 0; i0 < nlon; i0 += 8)
      for (int32_t j0 = 0; j0 < nlat; j0 += 8)
        for (int32_t i = i0; i < std::min(nlon, i0 + 8); ++i)
          for (int32_t j = j0; j < std::min(nlat, j0 + 8); ++j) {
            sky_map_direction(frame, lon_min, lon_max, lat_min, lat_max, nlon,
                              nlat, i, j, directions.data() + 3 * pixel.size());
            pixel.push_back((int64_t)i * nlat + j);
          }
    return CMI_GPU_OK;
  }
  void scatter(double *maps) const {
    for (size_t p = 0; p < nplanes; ++p)
      for (size_t k = 0; k < npixel; ++k)
        maps[p * npixel + (size_t)pixel[k]] = rays[p * npixel + k];
  }
};

/* ------------------------------------------------- continuum images -- */

/* f(std::integral_constant<int, FB>) for the channel block of the engine */
template <class F> void continuum_for_block(int fb, F &&f) {
  switch (fb) {
  case 4: f(std::integral_constant<int, 4>()); break;
  case 16: f(std::integral_constant<int, 16>()); break;
  default: f(std::integral_constant<int, 8>()); break;
  }
}

/* where the channels of a continuum call come from: the free-free
 * coefficients of the cells at freq[count], or the caller's
 * kappa[count][ncell] and source[count][ncell] (host). A source of records
 * like RecordSource, in batches of the engine's channel block. */
struct ContinuumInput {
  const double *freq = nullptr;
  const double *kappa = nullptr, *source = nullptr;
  int32_t count = 0;
  int fb = 0;
  /* device */
  double *records = nullptr, *dkappa = nullptr, *dsource = nullptr;
  unsigned int *ninvalid = nullptr;

  int batch() const { return fb; }
  /* the channels [c0, c0 + nc) of the caller's fields to the device */
  int upload(cmi_gpu_engine *e, int32_t c0, int32_t nc);
  /* counts the values out of range of the n uploaded ones */
  int count_invalid(cmi_gpu_engine *e, int64_t n);
  int begin(cmi_gpu_engine *e, const char *what, int32_t nf,
            RenderArena &arena);
  int records_of(cmi_gpu_engine *e, int32_t c0, int nc);
};

/* what every continuum call asks of its channels before a launch; nvalue is
 * the number of pixels or rays of one channel */
int continuum_check(const cmi_gpu_engine *e, const char *what, int32_t nf,
                    int64_t nvalue, const ContinuumInput &in,
                    const double *background) {
  if (nf < 1)
    return fail(CMI_GPU_EINVAL, "%s: at least one channel (%d asked for)",
                what, (int)nf);
  if ((int64_t)nf > (1ll << 28) || (int64_t)nf * nvalue > (1ll << 28))
    return fail(CMI_GPU_EINVAL, "%s: %d channels of %lld values: a call "
                "renders at most 2^28 values", what, (int)nf,
                (long long)nvalue);
  if (in.freq) {
    for (int32_t f = 0; f < nf; ++f)
      if (!std::isfinite(in.freq[f]) || !(in.freq[f] > 0.))
        return fail(CMI_GPU_EINVAL, "%s: frequency %d is not finite and "
                    "positive (%.17g)", what, (int)f, in.freq[f]);
    CMI_TRY(check_have_cells(e, what));
  }
  if (background)
    for (int32_t f = 0; f < nf; ++f)
      if (!std::isfinite(background[f]))
        return fail(CMI_GPU_EINVAL, "%s: the background of channel %d is not "
                    "finite", what, (int)f);
  return CMI_GPU_OK;
}

int ContinuumInput::upload(cmi_gpu_engine *e, int32_t c0, int32_t nc) {
  const size_t ncell = (size_t)e->ncell;
  HIP_TRY(hipMemcpy(dkappa, kappa + (size_t)c0 * ncell,
                    sizeof(double) * ncell * nc, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dsource, source + (size_t)c0 * ncell,
                    sizeof(double) * ncell * nc, hipMemcpyHostToDevice));
  return CMI_GPU_OK;
}

int ContinuumInput::count_invalid(cmi_gpu_engine *e, int64_t n) {
  continuum_field_check_kernel<<<grid_blocks(e, n, 8), 256, 0, e->stream>>>(
      dkappa, dsource, n, ninvalid);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

/* allocates the records (and the staging of the caller's fields) and refuses
 * fields with a value out of range: every block is uploaded and counted
 * before anything is marched. With one block it stays uploaded. */
int ContinuumInput::begin(cmi_gpu_engine *e, const char *what, int32_t nf,
                          RenderArena &arena) {
  const size_t ncell = (size_t)e->ncell;
  count = nf;
  fb = e->tune.continuum_channel_block;
  CMI_TRY(arena.alloc(records, 2 * ncell * fb));
  if (freq)
    return CMI_GPU_OK;
  const int nb = std::min<int>(nf, fb);
  CMI_TRY(arena.alloc(dkappa, ncell * nb));
  CMI_TRY(arena.alloc(dsource, ncell * nb));
  CMI_TRY(arena.alloc(ninvalid, 2));
  HIP_TRY(hipMemsetAsync(ninvalid, 0, 2 * sizeof(unsigned int), e->stream));
  for (int32_t c0 = 0; c0 < nf; c0 += fb) {
    const int32_t nc = std::min<int32_t>(fb, nf - c0);
    CMI_TRY(upload(e, c0, nc));
    CMI_TRY(count_invalid(e, (int64_t)ncell * nc));
  }
  unsigned int bad[2] = {0, 0};
  HIP_TRY(hipMemcpy(bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost));
  if (bad[0])
    return fail(CMI_GPU_EINVAL, "%s: %u absorption coefficient(s) are "
                "negative or not finite", what, bad[0]);
  if (bad[1])
    return fail(CMI_GPU_EINVAL, "%s: %u source function value(s) are not "
                "finite", what, bad[1]);
  return CMI_GPU_OK;
}

/* the records of the channels [c0, c0 + nc) onto the stream */
int ContinuumInput::records_of(cmi_gpu_engine *e, int32_t c0, int nc) {
  if (freq) {
    CellsDev *cells;
    CMI_TRY(cells_settled(e, cells));
    FreeFreeRecordArgs r;
    r.cells = *cells;
    r.ncell = e->ncell;
    r.helium_abundance = e->model.abundance[0];
    r.fb = fb;
    r.nfreq = nc;
    for (int f = 0; f < CMI_CONTINUUM_MAX_FB; ++f)
      r.freq[f] = f < nc ? freq[c0 + f] : 1.;
    r.records = records;
    free_free_record_kernel<<<grid_blocks(e, e->ncell, 8), 256, 0,
                              e->stream>>>(r);
  } else {
    /* (a single block is still there from the check) */
    if (count > fb)
      CMI_TRY(upload(e, c0, nc));
    field_continuum_record_kernel<<<(unsigned)((e->ncell + 255) / 256), 256, 0,
                                    e->stream>>>(dkappa, dsource, e->ncell, nc,
                                                 fb, records);
  }
  HIP_TRY(hipGetLastError());
  return CMI_GPU_OK;
}

/* the background of the channels [c0, c0 + nc) as a march launch takes it */
void continuum_background(const double *background, int32_t c0, int nc,
                          double *out) {
  for (int i = 0; i < CMI_CONTINUUM_MAX_FB; ++i)
    out[i] = (background && i < nc) ? background[c0 + i] : 0.;
}

/* images[nf][nx * ny] (host) of the parallel camera: per block of FB channels
 * the records, then per chunk of pixel rows one march launch */
int continuum_images(cmi_gpu_engine *e, const char *what, ContinuumInput &in,
                     int32_t nf, const double *background,
                     const LineViewDev &v, double *images) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  ParallelCamera cam;
  CMI_TRY(in.begin(e, what, nf, arena));
  const int fb = in.fb;
  /* (the sample buffer holds FB channels of a chunk's rows) */
  CMI_TRY(cam.begin(e, v,
                    e->tune.continuum_launch_rays
                        ? e->tune.continuum_launch_rays
                        : CMI_LINE_IMAGE_LAUNCH_SAMPLES / fb,
                    fb, std::min<int>(nf, fb), arena));
  return render_batches(e, in, [&](int32_t c0, int nc) -> int {
    CMI_TRY(cam.march([&]() -> int {
      ContinuumMarchArgs a;
      a.grid = e->grid;
      a.view = v;
      a.records = in.records;
      a.sx0 = cam.sx0();
      a.sx1 = cam.sx1();
      a.nc = nc;
      a.pad = 0;
      continuum_background(background, c0, nc, a.background);
      a.out = cam.out(0);
      a.channel_stride = cam.plane_stride();
      /* (with the tuning key timing the march launches are timed like the
       * transport launches: cmi_gpu_get_kernel_timing) */
      EventPair ev;
      CMI_TRY(timer_begin(e, ev));
      continuum_for_block(fb, [&](auto width) {
        continuum_march_kernel<decltype(width)::value>
            <<<cam.tiles(), 256, 0, e->stream>>>(a);
      });
      HIP_TRY(hipGetLastError());
      CMI_TRY(timer_end(e, e->kernel_events, ev,
                        (uint64_t)((a.sx1 - a.sx0) * cam.NY)));
      /* the images' reduction, channels in the place of lines */
      return cam.reduce(0, nc, 0);
    }));
    return cam.download(images + (size_t)c0 * cam.npixel, nc);
  });
}

/* out[nf][nrays] (host) of the rays from a point: per block of FB channels
 * the records, then per chunk of rays one march launch */
int continuum_sky(cmi_gpu_engine *e, const char *what, ContinuumInput &in,
                  int32_t nf, const double *background, const double *origin,
                  int64_t nrays, const double *directions, double *out) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  PointCamera cam;
  CMI_TRY(in.begin(e, what, nf, arena));
  const int fb = in.fb;
  CMI_TRY(cam.begin(e, origin, nrays, directions,
                    e->tune.continuum_launch_rays
                        ? e->tune.continuum_launch_rays
                        : CMI_SKY_LAUNCH_RAYS,
                    fb, arena));
  return render_batches(e, in, [&](int32_t c0, int nc) -> int {
    return cam.march(nc, out + (size_t)c0 * nrays, [&](int64_t n) -> int {
      ContinuumSkyMarchArgs a;
      a.grid = e->grid;
      for (int k = 0; k < 3; ++k)
        a.origin[k] = origin[k];
      a.directions = cam.directions;
      a.records = in.records;
      a.nrays = n;
      a.nc = nc;
      a.pad = 0;
      a.channel_stride = cam.chunk;
      a.out = cam.out;
      continuum_background(background, c0, nc, a.background);
      EventPair ev;
      CMI_TRY(timer_begin(e, ev));
      continuum_for_block(fb, [&](auto width) {
        continuum_sky_march_kernel<decltype(width)::value>
            <<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(a);
      });
      HIP_TRY(hipGetLastError());
      return timer_end(e, e->kernel_events, ev, (uint64_t)n);
    });
  });
}

/* --------------------------------------------- absorbing line cubes -- */

/* f(integral_constant<int, CB>, bool_constant<CALL>) for the channel block
 * and the expm1 form of the engine */
template <class F> void absorbing_for_variant(int cb, bool call, F &&f) {
  if (cb == 4) {
    if (call)
      f(std::integral_constant<int, 4>(), std::true_type());
    else
      f(std::integral_constant<int, 4>(), std::false_type());
  } else {
    if (call)
      f(std::integral_constant<int, 8>(), std::true_type());
    else
      f(std::integral_constant<int, 8>(), std::false_type());
  }
}

/* Where the records of an absorbing cube come from: the 21-cm line of the
 * cells as they are (hi set), or the caller's host fields a, sl, b[ncell]
 * with optional velocity[3][ncell] and {kc, sc}[ncell]. One record per cell
 * and call: begin() checks, uploads and writes them. */
struct AbsorbingInput {
  bool point = false; /* the layout: rays from a point */
  bool hi = false;
  double sigma_turb = 0.;
  int32_t spin_mode = CMI_HI_SPIN_KINETIC;
  const double *spin = nullptr; /* [1] or [ncell] (host) */
  bool free_free = true;
  const double *a = nullptr, *sl = nullptr, *b = nullptr, *velocity = nullptr,
               *kc = nullptr, *sc = nullptr;
  /* the direction to the observer, or the observer's velocity */
  double frame[3] = {0., 0., 0.};
  double dv = 1.;
  /* the background: [nchan] (host) or null, then one value for all */
  const double *background = nullptr;
  double background_all = 0.;
  double *records = nullptr; /* device */

  int doubles() const { return point ? 8 : 6; }
  int begin(cmi_gpu_engine *e, const char *what, RenderArena &arena);
  /* the background of the channels [c0, c0 + nc) as a march launch takes it */
  void background_of(int32_t c0, int nc, double *out) const {
    for (int i = 0; i < CMI_ABSORBING_MAX_CB; ++i)
      out[i] = i < nc ? (background ? background[c0 + i] : background_all) : 0.;
  }
};

/* what the H I calls ask of their arguments before anything is uploaded */
int hi_check(const cmi_gpu_engine *e, const char *what, double sigma_turb,
             int32_t spin_mode, const double *spin_temperature,
             double background_temperature) {
  CMI_TRY(check_sigma_turb(what, sigma_turb));
  if (spin_mode != CMI_HI_SPIN_KINETIC && spin_mode != CMI_HI_SPIN_FIXED &&
      spin_mode != CMI_HI_SPIN_CELLS)
    return fail(CMI_GPU_EINVAL, "%s: no spin temperature mode %d", what,
                (int)spin_mode);
  if (spin_mode != CMI_HI_SPIN_KINETIC && !spin_temperature)
    return fail(CMI_GPU_EINVAL, "%s: this spin temperature mode needs a spin "
                "temperature", what);
  if (spin_mode == CMI_HI_SPIN_FIXED &&
      (!(spin_temperature[0] > 0.) || !std::isfinite(spin_temperature[0])))
    return fail(CMI_GPU_EINVAL, "%s: the spin temperature must be positive "
                "and finite (%.17g)", what, spin_temperature[0]);
  if (!(background_temperature >= 0.) || !std::isfinite(background_temperature))
    return fail(CMI_GPU_EINVAL, "%s: the background temperature must be >= 0 "
                "and finite", what);
  /* (the render calls have refused a block with their view or rays; the
   * coefficients are what they march, so they are refused alike) */
  if (e->grid.decomposed)
    return fail(CMI_GPU_ESTATE, "%s: not available on a block of a decomposed "
                "grid", what);
  return check_have_cells(e, what);
}

/* B_nu10(T) on the host in the contract's form; 0 for T == 0 */
double hi_background(double T) {
  if (!(T > 0.))
    return 0.;
  const double nu = CMI_HI_FREQUENCY;
  const double x = (CMI_PLANCK * nu) / (CMI_BOLTZMANN * T);
  return (2. * CMI_PLANCK * nu * nu * nu / (CMI_LIGHTSPEED * CMI_LIGHTSPEED)) /
         std::expm1(x);
}

/* the caller's background[nchan], or null */
int absorbing_check_background(const char *what, const double *background,
                               int32_t nchan) {
  if (background)
    for (int32_t c = 0; c < nchan; ++c)
      if (!std::isfinite(background[c]))
        return fail(CMI_GPU_EINVAL, "%s: the background of channel %d is not "
                    "finite", what, (int)c);
  return CMI_GPU_OK;
}

int AbsorbingInput::begin(cmi_gpu_engine *e, const char *what,
                          RenderArena &arena) {
  const size_t ncell = (size_t)e->ncell;
  if (hi) {
    CellsDev *cells;
    CMI_TRY(cells_settled(e, cells));
    HiRecordArgs r;
    r.cells = *cells;
    r.ncell = e->ncell;
    r.helium_abundance = e->model.abundance[0];
    r.weight = cmi_emission_atomic_weight[0];
    r.sigma_turb = sigma_turb;
    r.dv = dv;
    r.spin_fixed = spin_mode == CMI_HI_SPIN_FIXED ? spin[0] : 0.;
    r.spin_cells = nullptr;
    if (spin_mode == CMI_HI_SPIN_CELLS) {
      double *dspin = nullptr;
      unsigned int bad = 0;
      CMI_TRY(arena.upload(dspin, spin, ncell));
      CMI_TRY(count_not_finite(e, dspin, (int64_t)ncell, bad));
      if (bad)
        return fail(CMI_GPU_EINVAL, "%s: %u spin temperature(s) are not "
                    "finite", what, bad);
      r.spin_cells = dspin;
    }
    r.spin_mode = spin_mode;
    r.free_free = free_free ? 1 : 0;
    for (int k = 0; k < 3; ++k)
      r.frame[k] = frame[k];
    r.velocity = e->cell_velocities;
    CMI_TRY(arena.alloc(records, ncell * doubles()));
    r.records = records;
    const int blocks = grid_blocks(e, e->ncell, 8);
    if (point)
      hi_record_kernel<true><<<blocks, 256, 0, e->stream>>>(r);
    else
      hi_record_kernel<false><<<blocks, 256, 0, e->stream>>>(r);
    HIP_TRY(hipGetLastError());
    /* finite cells can still overflow (a spin temperature of 1e-322 K gives
     * a = inf, and inf * 0 is NaN): the records are held to what the
     * caller's fields are held to */
    unsigned int *ninvalid = nullptr;
    unsigned int bad = 0;
    CMI_TRY(arena.alloc(ninvalid, 1));
    HIP_TRY(hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream));
    if (point)
      hi_record_check_kernel<true><<<blocks, 256, 0, e->stream>>>(
          records, e->ncell, ninvalid);
    else
      hi_record_check_kernel<false><<<blocks, 256, 0, e->stream>>>(
          records, e->ncell, ninvalid);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (bad)
      return fail(CMI_GPU_EINVAL, "%s: %u cell(s) have a 21-cm coefficient "
                  "that is not finite (a / dv, b, sl, kc, sc or sl - sc; a "
                  "spin temperature too close to 0 does that)", what, bad);
    return CMI_GPU_OK;
  }
  FieldAbsorbingRecordArgs r;
  double *da = nullptr, *dsl = nullptr, *db = nullptr, *dkc = nullptr,
         *dsc = nullptr, *dvelocity = nullptr;
  unsigned int *ninvalid = nullptr;
  if (velocity) {
    CMI_TRY(arena.upload(dvelocity, velocity, 3 * ncell));
    CMI_TRY(line_cube_check_velocities(e, what, dvelocity, 3 * (int64_t)ncell));
  }
  CMI_TRY(arena.upload(da, a, ncell));
  CMI_TRY(arena.upload(dsl, sl, ncell));
  CMI_TRY(arena.upload(db, b, ncell));
  if (kc) {
    CMI_TRY(arena.upload(dkc, kc, ncell));
    CMI_TRY(arena.upload(dsc, sc, ncell));
  }
  r.a = da;
  r.sl = dsl;
  r.b = db;
  r.kc = dkc;
  r.sc = dsc;
  r.velocity = dvelocity;
  r.ncell = e->ncell;
  r.dv = dv;
  for (int k = 0; k < 3; ++k)
    r.frame[k] = frame[k];
  r.records = nullptr;
  CMI_TRY(arena.alloc(ninvalid, 5));
  HIP_TRY(hipMemsetAsync(ninvalid, 0, 5 * sizeof(unsigned int), e->stream));
  absorbing_field_check_kernel<<<grid_blocks(e, e->ncell, 8), 256, 0,
                                 e->stream>>>(r, ninvalid);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  unsigned int bad[5] = {0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpy(bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost));
  if (bad[0])
    return fail(CMI_GPU_EINVAL, "%s: %u integrated line opacities are "
                "negative, not finite or not finite once divided by the "
                "channel width", what, bad[0]);
  if (bad[1])
    return fail(CMI_GPU_EINVAL, "%s: %u width(s) are negative or not finite",
                what, bad[1]);
  if (bad[2])
    return fail(CMI_GPU_EINVAL, "%s: %u continuum absorption coefficient(s) "
                "are negative or not finite", what, bad[2]);
  if (bad[3])
    return fail(CMI_GPU_EINVAL, "%s: %u line source function value(s) are not "
                "finite", what, bad[3]);
  if (bad[4])
    return fail(CMI_GPU_EINVAL, "%s: %u continuum source function value(s) "
                "are not finite, or not a finite distance from the line's",
                what, bad[4]);
  CMI_TRY(arena.alloc(records, ncell * doubles()));
  r.records = records;
  const unsigned blocks = (unsigned)((e->ncell + 255) / 256);
  if (point)
    field_absorbing_record_kernel<true><<<blocks, 256, 0, e->stream>>>(r);
  else
    field_absorbing_record_kernel<false><<<blocks, 256, 0, e->stream>>>(r);
  HIP_TRY(hipGetLastError());
  return CMI_GPU_OK;
}

/* what the general calls ask of their pointers */
int absorbing_check_fields(const char *what, const AbsorbingInput &in) {
  if (!in.a || !in.sl || !in.b)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  if ((in.kc == nullptr) != (in.sc == nullptr))
    return fail(CMI_GPU_EINVAL, "%s: the continuum opacity and source "
                "function come together or not at all", what);
  return CMI_GPU_OK;
}

/* cube[nchan][nx * ny] (host) of the parallel camera: the records, then per
 * chunk of pixel rows and block of CB channels one march launch */
int absorbing_cube(cmi_gpu_engine *e, const char *what, AbsorbingInput &in,
                   const LineCubeAxis &axis, const LineViewDev &v,
                   double *cube) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  ParallelCamera cam;
  in.point = false;
  in.dv = axis.dv;
  CMI_TRY(in.begin(e, what, arena));
  const int cb = e->tune.absorbing_cube_channel_block;
  const bool call = e->tune.absorbing_cube_expm1_call != 0;
  /* (the sample buffer holds CB channels of a chunk's rows) */
  CMI_TRY(cam.begin(e, v,
                    e->tune.absorbing_cube_launch_rays
                        ? e->tune.absorbing_cube_launch_rays
                        : CMI_LINE_IMAGE_LAUNCH_SAMPLES / cb,
                    cb, (size_t)axis.nchan, arena));
  CMI_TRY(cam.march([&]() -> int {
    for (int32_t c0 = 0; c0 < axis.nchan; c0 += cb) {
      AbsorbingMarchArgs a;
      a.grid = e->grid;
      a.view = v;
      a.records = in.records;
      a.sx0 = cam.sx0();
      a.sx1 = cam.sx1();
      a.c0 = c0;
      a.nc = std::min<int32_t>(cb, axis.nchan - c0);
      a.full = e->tune.absorbing_cube_window_skip ? 0 : 1;
      a.pad = 0;
      a.vmin = axis.vmin;
      a.dv = axis.dv;
      a.channel_stride = cam.plane_stride();
      a.out = cam.out(c0);
      in.background_of(c0, a.nc, a.background);
      EventPair ev;
      CMI_TRY(timer_begin(e, ev));
      absorbing_for_variant(cb, call, [&](auto width, auto as_call) {
        absorbing_cube_march_kernel<decltype(width)::value,
                                    decltype(as_call)::value>
            <<<cam.tiles(), 256, 0, e->stream>>>(a);
      });
      HIP_TRY(hipGetLastError());
      CMI_TRY(timer_end(e, e->kernel_events, ev,
                        (uint64_t)((a.sx1 - a.sx0) * cam.NY)));
      CMI_TRY(cam.reduce(0, a.nc, c0));
    }
    return CMI_GPU_OK;
  }));
  return cam.download(cube, (size_t)axis.nchan);
}

/* out[nchan][nrays] (host) of the rays from a point: the records, then per
 * chunk of rays and block of CB channels one march launch */
int absorbing_sky_cube(cmi_gpu_engine *e, const char *what, AbsorbingInput &in,
                       const LineCubeAxis &axis, const double *origin,
                       int64_t nrays, const double *directions, double *out) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  PointCamera cam;
  in.point = true;
  in.dv = axis.dv;
  CMI_TRY(in.begin(e, what, arena));
  const int cb = e->tune.absorbing_cube_channel_block;
  const bool call = e->tune.absorbing_cube_expm1_call != 0;
  CMI_TRY(cam.begin(e, origin, nrays, directions,
                    e->tune.absorbing_cube_launch_rays
                        ? e->tune.absorbing_cube_launch_rays
                        : std::min<int64_t>(CMI_SKY_LAUNCH_RAYS,
                                            CMI_SKY_CUBE_LAUNCH_VALUES /
                                                axis.nchan),
                    (size_t)axis.nchan, arena));
  cam.one_copy = true;
  return cam.march((size_t)axis.nchan, out, [&](int64_t n) -> int {
    for (int32_t c0 = 0; c0 < axis.nchan; c0 += cb) {
      AbsorbingSkyMarchArgs a;
      a.grid = e->grid;
      for (int k = 0; k < 3; ++k)
        a.origin[k] = origin[k];
      a.directions = cam.directions;
      a.records = in.records;
      a.nrays = n;
      a.c0 = c0;
      a.nc = std::min<int32_t>(cb, axis.nchan - c0);
      a.full = e->tune.absorbing_cube_window_skip ? 0 : 1;
      a.pad = 0;
      a.vmin = axis.vmin;
      a.dv = axis.dv;
      a.channel_stride = cam.chunk;
      a.out = cam.out;
      in.background_of(c0, a.nc, a.background);
      EventPair ev;
      CMI_TRY(timer_begin(e, ev));
      absorbing_for_variant(cb, call, [&](auto width, auto as_call) {
        absorbing_sky_march_kernel<decltype(width)::value,
                                        decltype(as_call)::value>
            <<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(a);
      });
      HIP_TRY(hipGetLastError());
      CMI_TRY(timer_end(e, e->kernel_events, ev, (uint64_t)n));
    }
    return CMI_GPU_OK;
  });
}
} // namespace
} // extern "C++"

/* --------------------------------------------------- line images -- */

int cmi_gpu_render_line_images(cmi_gpu_engine *e, int32_t nlines,
                               const int32_t *lines, double theta, double phi,
                               int32_t nx, int32_t ny, const double *anchor,
                               const double *sides, int32_t supersample,
                               double dust_cross_section, double *images) {
  static const char *what = "render_line_images";
  if (!e || !lines || !images)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_lines(what, nlines, lines, false));
  CMI_TRY(check_dust_cross_section(what, dust_cross_section));
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  CMI_TRY(check_have_cells(e, what));
  RecordSource src;
  src.count = nlines;
  src.lines = lines;
  src.dust_cross_section = dust_cross_section;
  return render_images(e, what, src, v, images);
}

int cmi_gpu_render_field_images(cmi_gpu_engine *e, int32_t nfields,
                                const double *fields, double theta, double phi,
                                int32_t nx, int32_t ny, const double *anchor,
                                const double *sides, int32_t supersample,
                                const double *extinction, double *images) {
  static const char *what = "render_field_images";
  if (!e || !fields || !images)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_field_count(what, nfields));
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  RecordSource src;
  src.count = nfields;
  src.fields = fields;
  src.extinction = extinction;
  return render_images(e, what, src, v, images);
}

int cmi_gpu_line_image_probe(cmi_gpu_engine *e, double theta, double phi,
                             int64_t n, const double *xy, int32_t max_cells,
                             double *out) {
  static const char *what = "line_image_probe";
  if (!e || n < 0 || n > (1 << 24) || max_cells < 0 || (n && (!xy || !out)))
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  LineViewDev v;
  CMI_TRY(line_image_view(e, what, theta, phi, v));
  CMI_TRY(check_image_coordinates(what, n, xy));
  if (n == 0)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  double *dxy = nullptr, *drows = nullptr;
  const size_t nvalue = (3 + 2 * (size_t)max_cells) * (size_t)n;
  CMI_TRY(arena.alloc(drows, nvalue));
  CMI_TRY(arena.upload(dxy, xy, 2 * (size_t)n));
  HIP_TRY(hipMemsetAsync(drows, 0, sizeof(double) * nvalue, e->stream));
  line_image_probe_kernel<<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
      e->grid, v, dxy, n, max_cells, drows);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, drows, sizeof(double) * nvalue,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

/* ------------------------------------------------ spectral line cubes -- */

double cmi_gpu_emission_line_atomic_weight(int32_t line) {
  return (line < 0 || line >= CMI_NEMISSIONLINE)
             ? 0.
             : cmi_emission_atomic_weight[line];
}

int cmi_gpu_set_cell_velocities(cmi_gpu_engine *e, const double *velocities) {
  static const char *what = "set_cell_velocities";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  HIP_TRY(hipSetDevice(e->device));
  if (!velocities) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    (void)hipFree(e->cell_velocities);
    e->cell_velocities = nullptr;
    dust_cube_mark_stale(e, "the cell velocities were replaced");
    return CMI_GPU_OK;
  }
  const size_t n = 3 * (size_t)e->ncell;
  double *fresh = nullptr;
  HIP_TRY(hipMalloc(&fresh, sizeof(double) * n));
  hipError_t err =
      hipMemcpy(fresh, velocities, sizeof(double) * n, hipMemcpyHostToDevice);
  int rc = CMI_GPU_OK;
  if (err != hipSuccess)
    rc = fail(CMI_GPU_EDEVICE, "%s: upload failed: %s", what,
              hipGetErrorString(err));
  else
    rc = line_cube_check_velocities(e, what, fresh, (int64_t)n);
  if (rc) {
    /* the previous state is kept */
    (void)hipFree(fresh);
    return rc;
  }
  /* a cube launch may still be enqueued and reads the old array (with cube
   * mode off nothing enqueued does, and the call is what it was) */
  if (e->dust_cube.nchan) {
    const hipError_t busy = hipStreamSynchronize(e->stream);
    if (busy != hipSuccess) {
      (void)hipFree(fresh);
      HIP_TRY(busy);
    }
  }
  (void)hipFree(e->cell_velocities);
  e->cell_velocities = fresh;
  dust_cube_mark_stale(e, "the cell velocities were replaced");
  return CMI_GPU_OK;
}

int cmi_gpu_render_line_cube(cmi_gpu_engine *e, int32_t nlines,
                             const int32_t *lines, double theta, double phi,
                             int32_t nx, int32_t ny, const double *anchor,
                             const double *sides, int32_t supersample,
                             double dust_cross_section, int32_t nchan,
                             double vmin, double vmax, double sigma_turb,
                             double *cube) {
  static const char *what = "render_line_cube";
  if (!e || !lines || !cube)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_lines(what, nlines, lines, true));
  CMI_TRY(check_dust_cross_section(what, dust_cross_section));
  CMI_TRY(check_sigma_turb(what, sigma_turb));
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  LineCubeAxis axis;
  CMI_TRY(line_cube_axis(what, nlines, nx, ny, nchan, vmin, vmax, axis));
  CMI_TRY(check_have_cells(e, what));
  RecordSource src;
  src.layout = RECORDS_CUBE;
  src.count = nlines;
  src.lines = lines;
  src.dust_cross_section = dust_cross_section;
  src.sigma_turb = sigma_turb;
  src.set_frame(v.n);
  return render_cube(e, what, src, v, axis, cube);
}

int cmi_gpu_render_field_cube(cmi_gpu_engine *e, int32_t nfields,
                              const double *fields, const double *extinction,
                              const double *velocity, const double *widths,
                              double theta, double phi, int32_t nx, int32_t ny,
                              const double *anchor, const double *sides,
                              int32_t supersample, int32_t nchan, double vmin,
                              double vmax, double *cube) {
  static const char *what = "render_field_cube";
  if (!e || !fields || !widths || !cube)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_field_count(what, nfields));
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  LineCubeAxis axis;
  CMI_TRY(line_cube_axis(what, nfields, nx, ny, nchan, vmin, vmax, axis));
  CMI_TRY(check_widths(what, widths, (size_t)e->ncell, nfields));
  RecordSource src;
  src.layout = RECORDS_CUBE;
  src.count = nfields;
  src.fields = fields;
  src.widths = widths;
  src.extinction = extinction;
  src.velocity = velocity;
  src.set_frame(v.n);
  return render_cube(e, what, src, v, axis, cube);
}

/* ------------------------------------------------------- sky maps -- */

int cmi_gpu_render_line_sky(cmi_gpu_engine *e, int32_t nlines,
                            const int32_t *lines, const double *origin,
                            int64_t nrays, const double *directions,
                            double dust_cross_section, double *out) {
  static const char *what = "render_line_sky";
  if (!e || !lines || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_lines(what, nlines, lines, false));
  CMI_TRY(check_dust_cross_section(what, dust_cross_section));
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  CMI_TRY(check_have_cells(e, what));
  RecordSource src;
  src.count = nlines;
  src.lines = lines;
  src.dust_cross_section = dust_cross_section;
  return render_sky(e, what, src, origin, nrays, directions, out);
}

int cmi_gpu_render_field_sky(cmi_gpu_engine *e, int32_t nfields,
                             const double *fields, const double *origin,
                             int64_t nrays, const double *directions,
                             const double *extinction, double *out) {
  static const char *what = "render_field_sky";
  if (!e || !fields || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_field_count(what, nfields));
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  RecordSource src;
  src.count = nfields;
  src.fields = fields;
  src.extinction = extinction;
  return render_sky(e, what, src, origin, nrays, directions, out);
}

int cmi_gpu_sky_probe(cmi_gpu_engine *e, const double *origin, int64_t n,
                      const double *directions, int32_t max_cells,
                      double *out) {
  static const char *what = "sky_probe";
  if (!e || !out || max_cells < 0)
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  CMI_TRY(sky_check(e, what, origin, n, 1ll << 24, directions));
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  double *ddir = nullptr, *drows = nullptr;
  const size_t nvalue = (3 + 2 * (size_t)max_cells) * (size_t)n;
  CMI_TRY(arena.alloc(drows, nvalue));
  CMI_TRY(arena.upload(ddir, directions, 3 * (size_t)n));
  HIP_TRY(hipMemsetAsync(drows, 0, sizeof(double) * nvalue, e->stream));
  sky_probe_kernel<<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
      e->grid, origin[0], origin[1], origin[2], ddir, n, max_cells, drows);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, drows, sizeof(double) * nvalue,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

int cmi_gpu_sky_map_directions(const double *frame, double lon_min,
                               double lon_max, double lat_min, double lat_max,
                               int32_t nlon, int32_t nlat, double *directions,
                               double *solid_angles) {
  static const char *what = "sky_map_directions";
  CMI_TRY(sky_map_check(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                        nlat));
  const double dl = (lon_max - lon_min) / nlon;
  for (int32_t i = 0; i < nlon; ++i)
    for (int32_t j = 0; j < nlat; ++j) {
      const size_t p = (size_t)i * nlat + j;
      if (directions)
        sky_map_direction(frame, lon_min, lon_max, lat_min, lat_max, nlon,
                          nlat, i, j, directions + 3 * p);
      if (solid_angles) {
        const double b_lo = lat_min + (lat_max - lat_min) * j / nlat;
        const double b_hi = lat_min + (lat_max - lat_min) * (j + 1) / nlat;
        solid_angles[p] = dl * (std::sin(b_hi) - std::sin(b_lo));
      }
    }
  return CMI_GPU_OK;
}

int cmi_gpu_render_line_sky_map(cmi_gpu_engine *e, int32_t nlines,
                                const int32_t *lines, const double *origin,
                                const double *frame, double lon_min,
                                double lon_max, double lat_min, double lat_max,
                                int32_t nlon, int32_t nlat,
                                double dust_cross_section, double *maps) {
  static const char *what = "render_line_sky_map";
  if (!e || !lines || !maps || nlines < 1)
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  CMI_TRY(sky_map_check(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                        nlat));
  SkyMapRays map;
  CMI_TRY(map.begin(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                    nlat, (size_t)nlines));
  CMI_TRY(cmi_gpu_render_line_sky(e, nlines, lines, origin,
                                  (int64_t)map.npixel, map.directions.data(),
                                  dust_cross_section, map.rays.data()));
  map.scatter(maps);
  return CMI_GPU_OK;
}

/* ------------------------------------------------------ sky cubes -- */

int cmi_gpu_render_line_sky_cube(cmi_gpu_engine *e, int32_t nlines,
                                 const int32_t *lines, const double *origin,
                                 const double *observer_velocity,
                                 int64_t nrays, const double *directions,
                                 double dust_cross_section, int32_t nchan,
                                 double vmin, double vmax, double sigma_turb,
                                 double *out) {
  static const char *what = "render_line_sky_cube";
  if (!e || !lines || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_lines(what, nlines, lines, true));
  CMI_TRY(check_dust_cross_section(what, dust_cross_section));
  CMI_TRY(check_sigma_turb(what, sigma_turb));
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  LineCubeAxis axis;
  RecordSource src;
  CMI_TRY(sky_cube_check(what, nlines, nrays, nchan, vmin, vmax,
                         observer_velocity, axis, src.frame));
  CMI_TRY(check_have_cells(e, what));
  src.layout = RECORDS_SKY_CUBE;
  src.count = nlines;
  src.lines = lines;
  src.dust_cross_section = dust_cross_section;
  src.sigma_turb = sigma_turb;
  return render_sky_cube(e, what, src, origin, nrays, directions, axis, out);
}

int cmi_gpu_render_field_sky_cube(cmi_gpu_engine *e, int32_t nfields,
                                  const double *fields,
                                  const double *extinction,
                                  const double *velocity, const double *widths,
                                  const double *origin,
                                  const double *observer_velocity,
                                  int64_t nrays, const double *directions,
                                  int32_t nchan, double vmin, double vmax,
                                  double *out) {
  static const char *what = "render_field_sky_cube";
  if (!e || !fields || !widths || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_field_count(what, nfields));
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  LineCubeAxis axis;
  RecordSource src;
  CMI_TRY(sky_cube_check(what, nfields, nrays, nchan, vmin, vmax,
                         observer_velocity, axis, src.frame));
  CMI_TRY(check_widths(what, widths, (size_t)e->ncell, nfields));
  src.layout = RECORDS_SKY_CUBE;
  src.count = nfields;
  src.fields = fields;
  src.widths = widths;
  src.extinction = extinction;
  src.velocity = velocity;
  return render_sky_cube(e, what, src, origin, nrays, directions, axis, out);
}

int cmi_gpu_render_line_sky_map_cube(cmi_gpu_engine *e, int32_t nlines,
                                     const int32_t *lines,
                                     const double *origin, const double *frame,
                                     double lon_min, double lon_max,
                                     double lat_min, double lat_max,
                                     int32_t nlon, int32_t nlat,
                                     double dust_cross_section,
                                     const double *observer_velocity,
                                     int32_t nchan, double vmin, double vmax,
                                     double sigma_turb, double *cubes) {
  static const char *what = "render_line_sky_map_cube";
  if (!e || !lines || !cubes || nlines < 1)
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  CMI_TRY(sky_map_check(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                        nlat));
  const int64_t npixel = (int64_t)nlon * nlat;
  if (nchan >= 1 && ((int64_t)nlines * nchan > (1ll << 28) ||
                     (int64_t)nlines * nchan * npixel > (1ll << 28)))
    return fail(CMI_GPU_EINVAL, "%s: %d x %d channels of %d x %d pixels: a "
                "cube has at most 2^28 values", what, (int)nlines, (int)nchan,
                (int)nlon, (int)nlat);
  SkyMapRays map;
  CMI_TRY(map.begin(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                    nlat,
                    (size_t)nlines * (size_t)std::max<int32_t>(nchan, 1)));
  CMI_TRY(cmi_gpu_render_line_sky_cube(
      e, nlines, lines, origin, observer_velocity, npixel,
      map.directions.data(), dust_cross_section, nchan, vmin, vmax, sigma_turb,
      map.rays.data()));
  map.scatter(cubes);
  return CMI_GPU_OK;
}

/* ------------------------------------------------- continuum images -- */

int cmi_gpu_free_free_coefficients(cmi_gpu_engine *e, int32_t nf,
                                   const double *freq, double *kappa_out,
                                   double *source_out) {
  static const char *what = "free_free_coefficients";
  if (!e || !freq || !kappa_out || !source_out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  ContinuumInput in;
  in.freq = freq;
  CMI_TRY(continuum_check(e, what, nf, 1, in, nullptr));
  HIP_TRY(hipSetDevice(e->device));
  const size_t ncell = (size_t)e->ncell;
  RenderArena arena;
  CMI_TRY(in.begin(e, what, nf, arena));
  const size_t fb = (size_t)in.fb;
  std::vector<double> host;
  try {
    host.resize(2 * ncell * fb);
  } catch (const std::bad_alloc &) {
    return fail(CMI_GPU_ENOMEM, "%s: out of host memory", what);
  }
  return render_batches(e, in, [&](int32_t c0, int nc) -> int {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(host.data(), in.records, sizeof(double) * 2 * ncell * fb,
                      hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < nc; ++i)
      for (size_t c = 0; c < ncell; ++c) {
        kappa_out[(size_t)(c0 + i) * ncell + c] = host[2 * (c * fb + i)];
        source_out[(size_t)(c0 + i) * ncell + c] = host[2 * (c * fb + i) + 1];
      }
    return CMI_GPU_OK;
  });
}

int cmi_gpu_render_continuum_images(cmi_gpu_engine *e, int32_t nf,
                                    const double *freq,
                                    const double *background, double theta,
                                    double phi, int32_t nx, int32_t ny,
                                    const double *anchor, const double *sides,
                                    int32_t supersample, double *out) {
  static const char *what = "render_continuum_images";
  if (!e || !freq || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  ContinuumInput in;
  in.freq = freq;
  CMI_TRY(continuum_check(e, what, nf, (int64_t)nx * ny, in, background));
  return continuum_images(e, what, in, nf, background, v, out);
}

int cmi_gpu_render_field_continuum_images(
    cmi_gpu_engine *e, int32_t nf, const double *kappa, const double *source,
    const double *background, double theta, double phi, int32_t nx,
    int32_t ny, const double *anchor, const double *sides,
    int32_t supersample, double *out) {
  static const char *what = "render_field_continuum_images";
  if (!e || !kappa || !source || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  ContinuumInput in;
  in.kappa = kappa;
  in.source = source;
  CMI_TRY(continuum_check(e, what, nf, (int64_t)nx * ny, in, background));
  return continuum_images(e, what, in, nf, background, v, out);
}

int cmi_gpu_render_continuum_sky(cmi_gpu_engine *e, int32_t nf,
                                 const double *freq, const double *background,
                                 const double *origin, int64_t nrays,
                                 const double *directions, double *out) {
  static const char *what = "render_continuum_sky";
  if (!e || !freq || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  ContinuumInput in;
  in.freq = freq;
  CMI_TRY(continuum_check(e, what, nf, nrays, in, background));
  return continuum_sky(e, what, in, nf, background, origin, nrays, directions,
                       out);
}

int cmi_gpu_render_field_continuum_sky(cmi_gpu_engine *e, int32_t nf,
                                       const double *kappa,
                                       const double *source,
                                       const double *background,
                                       const double *origin, int64_t nrays,
                                       const double *directions, double *out) {
  static const char *what = "render_field_continuum_sky";
  if (!e || !kappa || !source || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  ContinuumInput in;
  in.kappa = kappa;
  in.source = source;
  CMI_TRY(continuum_check(e, what, nf, nrays, in, background));
  return continuum_sky(e, what, in, nf, background, origin, nrays, directions,
                       out);
}

int cmi_gpu_render_continuum_sky_map(cmi_gpu_engine *e, int32_t nf,
                                     const double *freq,
                                     const double *background,
                                     const double *origin, int32_t nlon,
                                     int32_t nlat, const double *lon_range,
                                     const double *lat_range,
                                     const double *frame, double *out) {
  static const char *what = "render_continuum_sky_map";
  if (!e || !freq || !out || !lon_range || !lat_range)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(sky_map_check(what, frame, lon_range[0], lon_range[1], lat_range[0],
                        lat_range[1], nlon, nlat));
  const int64_t npixel = (int64_t)nlon * nlat;
  ContinuumInput in;
  in.freq = freq;
  CMI_TRY(continuum_check(e, what, nf, npixel, in, background));
  SkyMapRays map;
  CMI_TRY(map.begin(what, frame, lon_range[0], lon_range[1], lat_range[0],
                    lat_range[1], nlon, nlat, (size_t)nf));
  CMI_TRY(sky_check(e, what, origin, npixel, 1ll << 28,
                    map.directions.data()));
  CMI_TRY(continuum_sky(e, what, in, nf, background, origin, npixel,
                        map.directions.data(), map.rays.data()));
  map.scatter(out);
  return CMI_GPU_OK;
}

int cmi_gpu_continuum_probe(cmi_gpu_engine *e, int32_t nf, const double *kappa,
                            const double *source, const double *background,
                            int32_t point, const double *view, int64_t n,
                            const double *rays, int32_t max_cells,
                            double *out) {
  static const char *what = "continuum_probe";
  if (!e || !kappa || !source || !view || !out || max_cells < 0 ||
      (point != 0 && point != 1))
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  if (nf < 1 || nf > 1024)
    return fail(CMI_GPU_EINVAL, "%s: between 1 and 1024 channels (%d asked "
                "for)", what, (int)nf);
  LineViewDev v;
  double origin[3] = {0., 0., 0.};
  if (point) {
    CMI_TRY(sky_check(e, what, view, n, 1ll << 20, rays));
    for (int a = 0; a < 3; ++a)
      origin[a] = view[a];
    /* (not read by the kernel; set so that it is passed initialised) */
    std::memset(&v, 0, sizeof v);
  } else {
    if (n <= 0 || n > (1ll << 20) || !rays)
      return fail(CMI_GPU_EINVAL, "%s: between 1 and 2^20 rays (%lld asked "
                  "for)", what, (long long)n);
    CMI_TRY(line_image_view(e, what, view[0], view[1], v));
    CMI_TRY(check_image_coordinates(what, n, rays));
  }
  ContinuumInput in;
  in.kappa = kappa;
  in.source = source;
  CMI_TRY(continuum_check(e, what, nf, 1, in, background));
  HIP_TRY(hipSetDevice(e->device));
  const size_t ncell = (size_t)e->ncell;
  const size_t nvalue =
      (3 + (2 + (size_t)nf) * (size_t)max_cells + (size_t)nf) * (size_t)n;
  RenderArena arena;
  double *drays = nullptr, *drows = nullptr, *dbackground = nullptr;
  CMI_TRY(arena.alloc(in.dkappa, ncell * nf));
  CMI_TRY(arena.alloc(in.dsource, ncell * nf));
  CMI_TRY(arena.alloc(in.ninvalid, 2));
  CMI_TRY(arena.alloc(drows, nvalue));
  HIP_TRY(hipMemsetAsync(in.ninvalid, 0, 2 * sizeof(unsigned int), e->stream));
  CMI_TRY(in.upload(e, 0, nf));
  CMI_TRY(in.count_invalid(e, (int64_t)ncell * nf));
  unsigned int bad[2] = {0, 0};
  HIP_TRY(hipMemcpy(bad, in.ninvalid, sizeof bad, hipMemcpyDeviceToHost));
  if (bad[0] || bad[1])
    return fail(CMI_GPU_EINVAL, "%s: %u absorption coefficient(s) are "
                "negative or not finite, %u source function value(s) are not "
                "finite", what, bad[0], bad[1]);
  std::vector<double> bg((size_t)nf, 0.);
  if (background)
    std::copy(background, background + nf, bg.begin());
  CMI_TRY(arena.upload(dbackground, bg.data(), (size_t)nf));
  CMI_TRY(arena.upload(drays, rays, (point ? 3 : 2) * (size_t)n));
  HIP_TRY(hipMemsetAsync(drows, 0, sizeof(double) * nvalue, e->stream));
  continuum_probe_kernel<<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
      e->grid, v, point, origin[0], origin[1], origin[2], drays, n, in.dkappa,
      in.dsource, dbackground, nf, e->ncell, max_cells, drows);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, drows, sizeof(double) * nvalue,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

/* --------------------------------------------- absorbing line cubes -- */

int cmi_gpu_hi_coefficients(cmi_gpu_engine *e, double sigma_turb,
                            int32_t spin_mode, const double *spin_temperature,
                            int32_t free_free, double *a, double *sl,
                            double *b, double *kc, double *sc) {
  static const char *what = "hi_coefficients";
  if (!e || !a || !sl || !b || !kc || !sc)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(hi_check(e, what, sigma_turb, spin_mode, spin_temperature, 0.));
  HIP_TRY(hipSetDevice(e->device));
  const size_t ncell = (size_t)e->ncell;
  std::vector<double> host;
  try {
    host.resize(6 * ncell);
  } catch (const std::bad_alloc &) {
    return fail(CMI_GPU_ENOMEM, "%s: out of host memory", what);
  }
  RenderArena arena;
  AbsorbingInput in;
  in.hi = true;
  in.sigma_turb = sigma_turb;
  in.spin_mode = spin_mode;
  in.spin = spin_temperature;
  in.free_free = free_free != 0;
  /* (a / 1 is a) */
  in.dv = 1.;
  CMI_TRY(in.begin(e, what, arena));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(host.data(), in.records, sizeof(double) * 6 * ncell,
                    hipMemcpyDeviceToHost));
  for (size_t c = 0; c < ncell; ++c) {
    a[c] = host[6 * c];
    b[c] = host[6 * c + 2];
    sl[c] = host[6 * c + 3];
    kc[c] = host[6 * c + 4];
    sc[c] = host[6 * c + 5];
  }
  return CMI_GPU_OK;
}

int cmi_gpu_render_hi_cube(cmi_gpu_engine *e, double theta, double phi,
                           int32_t nx, int32_t ny, const double *anchor,
                           const double *sides, int32_t supersample,
                           int32_t nchan, double vmin, double vmax,
                           double sigma_turb, int32_t spin_mode,
                           const double *spin_temperature, int32_t free_free,
                           double background_temperature, double *cube) {
  static const char *what = "render_hi_cube";
  if (!e || !cube)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  LineCubeAxis axis;
  CMI_TRY(line_cube_axis(what, 1, nx, ny, nchan, vmin, vmax, axis));
  CMI_TRY(hi_check(e, what, sigma_turb, spin_mode, spin_temperature,
                   background_temperature));
  AbsorbingInput in;
  in.hi = true;
  in.sigma_turb = sigma_turb;
  in.spin_mode = spin_mode;
  in.spin = spin_temperature;
  in.free_free = free_free != 0;
  in.background_all = hi_background(background_temperature);
  for (int k = 0; k < 3; ++k)
    in.frame[k] = v.n[k];
  return absorbing_cube(e, what, in, axis, v, cube);
}

int cmi_gpu_render_hi_sky_cube(cmi_gpu_engine *e, const double *origin,
                               const double *observer_velocity, int64_t nrays,
                               const double *directions, int32_t nchan,
                               double vmin, double vmax, double sigma_turb,
                               int32_t spin_mode,
                               const double *spin_temperature,
                               int32_t free_free,
                               double background_temperature, double *out) {
  static const char *what = "render_hi_sky_cube";
  if (!e || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  LineCubeAxis axis;
  AbsorbingInput in;
  CMI_TRY(sky_cube_check(what, 1, nrays, nchan, vmin, vmax, observer_velocity,
                         axis, in.frame));
  CMI_TRY(hi_check(e, what, sigma_turb, spin_mode, spin_temperature,
                   background_temperature));
  in.hi = true;
  in.sigma_turb = sigma_turb;
  in.spin_mode = spin_mode;
  in.spin = spin_temperature;
  in.free_free = free_free != 0;
  in.background_all = hi_background(background_temperature);
  return absorbing_sky_cube(e, what, in, axis, origin, nrays, directions, out);
}

int cmi_gpu_render_hi_sky_map_cube(
    cmi_gpu_engine *e, const double *origin, const double *frame,
    double lon_min, double lon_max, double lat_min, double lat_max,
    int32_t nlon, int32_t nlat, const double *observer_velocity,
    int32_t nchan, double vmin, double vmax, double sigma_turb,
    int32_t spin_mode, const double *spin_temperature, int32_t free_free,
    double background_temperature, double *cube) {
  static const char *what = "render_hi_sky_map_cube";
  if (!e || !cube)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(sky_map_check(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                        nlat));
  const int64_t npixel = (int64_t)nlon * nlat;
  if (nchan >= 1 &&
      (nchan > (1 << 28) || (int64_t)nchan * npixel > (1ll << 28)))
    return fail(CMI_GPU_EINVAL, "%s: %d channels of %d x %d pixels: a cube has "
                "at most 2^28 values", what, (int)nchan, (int)nlon, (int)nlat);
  SkyMapRays map;
  CMI_TRY(map.begin(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                    nlat, (size_t)std::max<int32_t>(nchan, 1)));
  CMI_TRY(cmi_gpu_render_hi_sky_cube(
      e, origin, observer_velocity, npixel, map.directions.data(), nchan, vmin,
      vmax, sigma_turb, spin_mode, spin_temperature, free_free,
      background_temperature, map.rays.data()));
  map.scatter(cube);
  return CMI_GPU_OK;
}

int cmi_gpu_render_field_absorbing_cube(
    cmi_gpu_engine *e, const double *a, const double *sl, const double *b,
    const double *velocity, const double *kc, const double *sc,
    const double *background, double theta, double phi, int32_t nx,
    int32_t ny, const double *anchor, const double *sides,
    int32_t supersample, int32_t nchan, double vmin, double vmax,
    double *cube) {
  static const char *what = "render_field_absorbing_cube";
  if (!e || !cube)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  AbsorbingInput in;
  in.a = a;
  in.sl = sl;
  in.b = b;
  in.velocity = velocity;
  in.kc = kc;
  in.sc = sc;
  in.background = background;
  CMI_TRY(absorbing_check_fields(what, in));
  LineViewDev v;
  CMI_TRY(line_image_geometry(e, what, theta, phi, nx, ny, anchor, sides,
                              supersample, v));
  LineCubeAxis axis;
  CMI_TRY(line_cube_axis(what, 1, nx, ny, nchan, vmin, vmax, axis));
  CMI_TRY(absorbing_check_background(what, background, nchan));
  for (int k = 0; k < 3; ++k)
    in.frame[k] = v.n[k];
  return absorbing_cube(e, what, in, axis, v, cube);
}

int cmi_gpu_render_field_absorbing_sky_cube(
    cmi_gpu_engine *e, const double *a, const double *sl, const double *b,
    const double *velocity, const double *kc, const double *sc,
    const double *background, const double *origin,
    const double *observer_velocity, int64_t nrays, const double *directions,
    int32_t nchan, double vmin, double vmax, double *out) {
  static const char *what = "render_field_absorbing_sky_cube";
  if (!e || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  AbsorbingInput in;
  in.a = a;
  in.sl = sl;
  in.b = b;
  in.velocity = velocity;
  in.kc = kc;
  in.sc = sc;
  in.background = background;
  CMI_TRY(absorbing_check_fields(what, in));
  CMI_TRY(sky_check(e, what, origin, nrays, 1ll << 28, directions));
  LineCubeAxis axis;
  CMI_TRY(sky_cube_check(what, 1, nrays, nchan, vmin, vmax, observer_velocity,
                         axis, in.frame));
  CMI_TRY(absorbing_check_background(what, background, nchan));
  return absorbing_sky_cube(e, what, in, axis, origin, nrays, directions, out);
}

int cmi_gpu_absorbing_cube_probe(
    cmi_gpu_engine *e, const double *a, const double *sl, const double *b,
    const double *velocity, const double *kc, const double *sc,
    const double *background, int32_t nchan, double vmin, double vmax,
    int32_t point, const double *view, const double *observer_velocity,
    int64_t n, const double *rays, int32_t max_cells, double *out) {
  static const char *what = "absorbing_cube_probe";
  if (!e || !view || !out || max_cells < 0 || (point != 0 && point != 1))
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  if (nchan < 1 || nchan > 1024)
    return fail(CMI_GPU_EINVAL, "%s: between 1 and 1024 channels (%d asked "
                "for)", what, (int)nchan);
  AbsorbingInput in;
  in.a = a;
  in.sl = sl;
  in.b = b;
  in.velocity = velocity;
  in.kc = kc;
  in.sc = sc;
  in.point = point != 0;
  CMI_TRY(absorbing_check_fields(what, in));
  LineViewDev v;
  LineCubeAxis axis;
  double origin[3] = {0., 0., 0.};
  if (point) {
    CMI_TRY(sky_check(e, what, view, n, 1ll << 20, rays));
    CMI_TRY(sky_cube_check(what, 1, n, nchan, vmin, vmax, observer_velocity,
                           axis, in.frame));
    for (int k = 0; k < 3; ++k)
      origin[k] = view[k];
    /* (not read by the kernel; set so that it is passed initialised) */
    std::memset(&v, 0, sizeof v);
  } else {
    if (n <= 0 || n > (1ll << 20) || !rays)
      return fail(CMI_GPU_EINVAL, "%s: between 1 and 2^20 rays (%lld asked "
                  "for)", what, (long long)n);
    CMI_TRY(line_image_view(e, what, view[0], view[1], v));
    CMI_TRY(check_image_coordinates(what, n, rays));
    CMI_TRY(line_cube_axis(what, 1, 1, 1, nchan, vmin, vmax, axis));
    for (int k = 0; k < 3; ++k)
      in.frame[k] = v.n[k];
  }
  CMI_TRY(absorbing_check_background(what, background, nchan));
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  in.dv = axis.dv;
  CMI_TRY(in.begin(e, what, arena));
  const size_t nvalue =
      (3 + (2 + (size_t)nchan) * (size_t)max_cells + (size_t)nchan) *
      (size_t)n;
  double *drays = nullptr, *drows = nullptr, *dbackground = nullptr;
  std::vector<double> bg((size_t)nchan, 0.);
  if (background)
    std::copy(background, background + nchan, bg.begin());
  CMI_TRY(arena.alloc(drows, nvalue));
  CMI_TRY(arena.upload(dbackground, bg.data(), (size_t)nchan));
  CMI_TRY(arena.upload(drays, rays, (point ? 3 : 2) * (size_t)n));
  HIP_TRY(hipMemsetAsync(drows, 0, sizeof(double) * nvalue, e->stream));
  absorbing_cube_probe_kernel<<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
      e->grid, v, point, origin[0], origin[1], origin[2], drays, n, in.records,
      dbackground, nchan, axis.vmin, axis.dv, max_cells, drows);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, drows, sizeof(double) * nvalue,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

/* ---------------------------------------------- absorption spectra -- */

extern "C++" {
namespace {
/* The lines of an absorption call: K constants S and g, and the densities and
 * widths either of the caller (n, b: host [K][ncell]) or built from the cells
 * (ions, weights, sigma_turb). begin() checks, uploads and writes the records
 * {n, b}[K][ncell] and {w, 0}[ncell]. */
struct AbsorptionInput {
  int32_t nlines = 0;
  const double *S = nullptr, *g = nullptr;
  const double *n = nullptr, *b = nullptr, *velocity = nullptr;
  const int32_t *ions = nullptr;
  const double *weights = nullptr;
  double sigma_turb = 0.;
  bool from_cells = false;
  double v_obs[3] = {0., 0., 0.};
  double2 *records = nullptr;
  double *velocity_records = nullptr, *dS = nullptr, *dg = nullptr;

  int check(const cmi_gpu_engine *e, const char *what) const;
  int begin(cmi_gpu_engine *e, const char *what, RenderArena &arena);
};

int AbsorptionInput::check(const cmi_gpu_engine *e, const char *what) const {
  if (nlines < 1 || nlines > CMI_ABSORPTION_MAX_LINES)
    return fail(CMI_GPU_EINVAL, "%s: between 1 and %d lines (%d asked for)",
                what, CMI_ABSORPTION_MAX_LINES, (int)nlines);
  if (!S || !g)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  for (int32_t l = 0; l < nlines; ++l) {
    if (!(S[l] >= 0.) || !std::isfinite(S[l]))
      return fail(CMI_GPU_EINVAL, "%s: the integrated cross section of line "
                  "%d is negative or not finite", what, (int)l);
    if (!(g[l] >= 0.) || !std::isfinite(g[l]))
      return fail(CMI_GPU_EINVAL, "%s: the damping width of line %d is "
                  "negative or not finite", what, (int)l);
  }
  if (from_cells) {
    if (!ions || !weights)
      return fail(CMI_GPU_EINVAL, "%s: null argument", what);
    for (int32_t l = 0; l < nlines; ++l) {
      if (ions[l] < 0 || ions[l] >= CMI_NION)
        return fail(CMI_GPU_EINVAL, "%s: no ion %d", what, (int)ions[l]);
      if (!(weights[l] > 0.) || !std::isfinite(weights[l]))
        return fail(CMI_GPU_EINVAL, "%s: the atomic weight of line %d must be "
                    "positive and finite", what, (int)l);
    }
    CMI_TRY(check_sigma_turb(what, sigma_turb));
    CMI_TRY(check_have_cells(e, what));
  } else if (!n || !b) {
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  }
  return CMI_GPU_OK;
}

int AbsorptionInput::begin(cmi_gpu_engine *e, const char *what,
                           RenderArena &arena) {
  const size_t ncell = (size_t)e->ncell;
  const int64_t count = (int64_t)nlines * e->ncell;
  const double *dvelocity = nullptr;
  CMI_TRY(arena.upload(dS, S, (size_t)nlines));
  CMI_TRY(arena.upload(dg, g, (size_t)nlines));
  CMI_TRY(arena.alloc(records, (size_t)count));
  if (from_cells) {
    CellsDev *cells;
    CMI_TRY(cells_settled(e, cells));
    AbsorptionIonRecordArgs r;
    r.cells = *cells;
    r.ncell = e->ncell;
    r.nlines = nlines;
    for (int32_t l = 0; l < nlines; ++l) {
      const int el = cmi_absorption_ion_element[ions[l]];
      r.ion[l] = ions[l];
      r.abundance[l] = el < 0 ? 1. : e->model.abundance[el];
      r.weight[l] = weights[l];
    }
    r.sigma_turb = sigma_turb;
    r.records = records;
    absorption_ion_record_kernel<<<(unsigned)((e->ncell + 255) / 256), 256, 0,
                                   e->stream>>>(r);
    HIP_TRY(hipGetLastError());
    dvelocity = e->cell_velocities;
  } else {
    double *dn = nullptr, *db = nullptr, *dvel = nullptr;
    if (velocity) {
      CMI_TRY(arena.upload(dvel, velocity, 3 * ncell));
      CMI_TRY(line_cube_check_velocities(e, what, dvel, 3 * (int64_t)ncell));
      dvelocity = dvel;
    }
    CMI_TRY(arena.upload(dn, n, (size_t)count));
    CMI_TRY(arena.upload(db, b, (size_t)count));
    field_absorption_record_kernel<<<(unsigned)((count + 255) / 256), 256, 0,
                                     e->stream>>>(dn, db, count, records);
    HIP_TRY(hipGetLastError());
  }
  unsigned int *ninvalid = nullptr;
  unsigned int bad[3] = {0, 0, 0};
  CMI_TRY(arena.alloc(ninvalid, 3));
  HIP_TRY(hipMemsetAsync(ninvalid, 0, sizeof bad, e->stream));
  absorption_record_check_kernel<<<grid_blocks(e, e->ncell, 8), 256, 0,
                                   e->stream>>>(records, dg, e->ncell, nlines,
                                                ninvalid);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (bad[0])
    return fail(CMI_GPU_EINVAL, "%s: %u absorber densities are negative or "
                "not finite", what, bad[0]);
  if (bad[1])
    return fail(CMI_GPU_EINVAL, "%s: %u Doppler width(s) are negative or not "
                "finite", what, bad[1]);
  if (bad[2])
    return fail(CMI_GPU_EINVAL, "%s: %u cell(s) of a damped line hold "
                "absorbers of Doppler width 0 (a = g / b has no value)", what,
                bad[2]);
  CMI_TRY(arena.alloc(velocity_records, 4 * ncell));
  absorption_velocity_record_kernel<<<(unsigned)((e->ncell + 255) / 256), 256,
                                      0, e->stream>>>(
      dvelocity, v_obs[0], v_obs[1], v_obs[2], e->ncell, velocity_records);
  HIP_TRY(hipGetLastError());
  return CMI_GPU_OK;
}

/* what an absorption call asks of the engine and of its sightlines */
int absorption_check_rays(const cmi_gpu_engine *e, const char *what,
                          int64_t nrays, int64_t max_rays,
                          const double *origins, const double *directions,
                          const double *lengths) {
  if (!origins || !lengths)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  /* (the grid, the count and the directions as every sky call has them
   * checked; the origin it looks at is the first ray's) */
  CMI_TRY(sky_check(e, what, origins, nrays, max_rays, directions));
  for (int64_t r = 0; r < nrays; ++r) {
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(origins[3 * r + a]))
        return fail(CMI_GPU_EINVAL, "%s: component %d of the origin of ray "
                    "%lld is not finite", what, a, (long long)r);
    if (!(lengths[r] > 0.))
      return fail(CMI_GPU_EINVAL, "%s: the length of ray %lld must be "
                  "positive (+inf: to the edge of the box)", what,
                  (long long)r);
  }
  return CMI_GPU_OK;
}

template <class F> void absorption_for_variant(int rows, bool share, F &&f) {
  if (rows == 1) {
    if (share)
      f(std::integral_constant<int, 1>(), std::true_type());
    else
      f(std::integral_constant<int, 1>(), std::false_type());
  } else if (rows == 2) {
    if (share)
      f(std::integral_constant<int, 2>(), std::true_type());
    else
      f(std::integral_constant<int, 2>(), std::false_type());
  } else {
    if (share)
      f(std::integral_constant<int, 4>(), std::true_type());
    else
      f(std::integral_constant<int, 4>(), std::false_type());
  }
}

/* tau[nrays][K][nchan] and N[nrays][K] (host): the records, one launch */
int absorption_spectra(cmi_gpu_engine *e, const char *what,
                       AbsorptionInput &in, const LineCubeAxis &axis,
                       int64_t nrays, const double *origins,
                       const double *directions, const double *lengths,
                       double *tau, double *N) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  CMI_TRY(in.begin(e, what, arena));
  int rows = e->tune.absorption_slab_rows;
  if (!rows)
    rows = axis.nchan <= 64 ? 1 : (axis.nchan <= 128 ? 2 : CMI_ABSORPTION_R);
  const size_t nrl = (size_t)nrays * (size_t)in.nlines;
  double *dorigins = nullptr, *ddirections = nullptr, *dlengths = nullptr,
         *dtau = nullptr, *dN = nullptr;
  CMI_TRY(arena.upload(dorigins, origins, 3 * (size_t)nrays));
  CMI_TRY(arena.upload(ddirections, directions, 3 * (size_t)nrays));
  CMI_TRY(arena.upload(dlengths, lengths, (size_t)nrays));
  CMI_TRY(arena.alloc(dtau, nrl * (size_t)axis.nchan));
  CMI_TRY(arena.alloc(dN, nrl));
  AbsorptionMarchArgs a;
  a.grid = e->grid;
  a.origins = dorigins;
  a.directions = ddirections;
  a.lengths = dlengths;
  a.velocity_records = in.velocity_records;
  a.records = in.records;
  a.S = in.dS;
  a.g = in.dg;
  a.ncell = e->ncell;
  a.nlines = (uint32_t)in.nlines;
  a.nslab = (uint32_t)((axis.nchan + 64 * rows - 1) / (64 * rows));
  /* (nrays K nchan <= 2^28 has been checked) */
  a.nitems = (uint32_t)(nrl * a.nslab);
  a.nchan = axis.nchan;
  a.full = e->tune.absorption_skips ? 0 : 1;
  a.pad = 0;
  a.vmin = axis.vmin;
  a.dv = axis.dv;
  a.tau = dtau;
  a.N = dN;
  EventPair ev;
  CMI_TRY(timer_begin(e, ev));
  absorption_for_variant(rows, e->tune.absorption_edge_sharing != 0,
                         [&](auto r, auto share) {
    absorption_march_kernel<decltype(r)::value, decltype(share)::value>
        <<<(a.nitems + 3) / 4, 256, 0, e->stream>>>(a);
  });
  HIP_TRY(hipGetLastError());
  CMI_TRY(timer_end(e, e->kernel_events, ev, (uint64_t)nrays));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(tau, dtau, sizeof(double) * nrl * (size_t)axis.nchan,
                    hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(N, dN, sizeof(double) * nrl, hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

/* the checks the two render calls share; *empty: zero rays, nothing to do */
int absorption_render_check(cmi_gpu_engine *e, const char *what,
                            const AbsorptionInput &in, int64_t nrays,
                            const double *origins, const double *directions,
                            const double *lengths,
                            const double *observer_velocity, int32_t nchan,
                            double vmin, double vmax, const double *tau,
                            const double *N, LineCubeAxis &axis,
                            double v_obs[3], bool &empty) {
  empty = false;
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(in.check(e, what));
  if (nrays == 0) {
    CMI_TRY(sky_cube_check(what, in.nlines, 1, nchan, vmin, vmax,
                           observer_velocity, axis, v_obs));
    empty = true;
    return CMI_GPU_OK;
  }
  if (!tau || !N)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(absorption_check_rays(e, what, nrays, 1ll << 24, origins, directions,
                                lengths));
  return sky_cube_check(what, in.nlines, nrays, nchan, vmin, vmax,
                        observer_velocity, axis, v_obs);
}
} // namespace
} // extern "C++"

int cmi_gpu_render_field_absorption_spectra(
    cmi_gpu_engine *e, int32_t nlines, const double *n, const double *b,
    const double *S, const double *g, const double *velocity, int64_t nrays,
    const double *origins, const double *directions, const double *lengths,
    const double *observer_velocity, int32_t nchan, double vmin, double vmax,
    double *tau, double *N) {
  static const char *what = "render_field_absorption_spectra";
  AbsorptionInput in;
  in.nlines = nlines;
  in.S = S;
  in.g = g;
  in.n = n;
  in.b = b;
  in.velocity = velocity;
  LineCubeAxis axis;
  bool empty;
  CMI_TRY(absorption_render_check(e, what, in, nrays, origins, directions,
                                  lengths, observer_velocity, nchan, vmin,
                                  vmax, tau, N, axis, in.v_obs, empty));
  if (empty)
    return CMI_GPU_OK;
  return absorption_spectra(e, what, in, axis, nrays, origins, directions,
                            lengths, tau, N);
}

int cmi_gpu_render_absorption_spectra(
    cmi_gpu_engine *e, int32_t nlines, const int32_t *ions,
    const double *weights, const double *S, const double *g,
    double sigma_turb, int64_t nrays, const double *origins,
    const double *directions, const double *lengths,
    const double *observer_velocity, int32_t nchan, double vmin, double vmax,
    double *tau, double *N) {
  static const char *what = "render_absorption_spectra";
  AbsorptionInput in;
  in.nlines = nlines;
  in.S = S;
  in.g = g;
  in.ions = ions;
  in.weights = weights;
  in.sigma_turb = sigma_turb;
  in.from_cells = true;
  LineCubeAxis axis;
  bool empty;
  CMI_TRY(absorption_render_check(e, what, in, nrays, origins, directions,
                                  lengths, observer_velocity, nchan, vmin,
                                  vmax, tau, N, axis, in.v_obs, empty));
  if (empty)
    return CMI_GPU_OK;
  return absorption_spectra(e, what, in, axis, nrays, origins, directions,
                            lengths, tau, N);
}

int cmi_gpu_absorption_probe(cmi_gpu_engine *e, const double *n,
                             const double *b, double S, double g,
                             const double *velocity, const double *origin,
                             const double *direction, double length,
                             const double *observer_velocity, int32_t nchan,
                             double vmin, double vmax, int32_t nprobe,
                             const int32_t *channels, int32_t max_cells,
                             double *out) {
  static const char *what = "absorption_probe";
  if (!e || !out || max_cells < 0 || nprobe < 0 ||
      nprobe > CMI_ABSORPTION_PROBE_CHANNELS || (nprobe > 0 && !channels))
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  AbsorptionInput in;
  in.nlines = 1;
  in.S = &S;
  in.g = &g;
  in.n = n;
  in.b = b;
  in.velocity = velocity;
  CMI_TRY(in.check(e, what));
  CMI_TRY(absorption_check_rays(e, what, 1, 1, origin, direction, &length));
  LineCubeAxis axis;
  CMI_TRY(sky_cube_check(what, 1, 1, nchan, vmin, vmax, observer_velocity,
                         axis, in.v_obs));
  for (int32_t k = 0; k < nprobe; ++k)
    if (channels[k] < 0 || channels[k] >= nchan)
      return fail(CMI_GPU_EINVAL, "%s: no channel %d", what, (int)channels[k]);
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  CMI_TRY(in.begin(e, what, arena));
  const size_t nvalue =
      3 + (2 + (size_t)nprobe) * (size_t)max_cells + (size_t)nprobe;
  const double ray[7] = {origin[0],    origin[1],    origin[2], direction[0],
                         direction[1], direction[2], length};
  double *dray = nullptr, *drow = nullptr;
  int32_t *dchannels = nullptr;
  CMI_TRY(arena.upload(dray, ray, 7));
  CMI_TRY(arena.alloc(drow, nvalue));
  CMI_TRY(arena.alloc(dchannels, CMI_ABSORPTION_PROBE_CHANNELS));
  if (nprobe)
    HIP_TRY(hipMemcpy(dchannels, channels, sizeof(int32_t) * nprobe,
                      hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(drow, 0, sizeof(double) * nvalue, e->stream));
  absorption_probe_kernel<<<1, 64, 0, e->stream>>>(
      e->grid, dray, in.velocity_records, in.records, S, g, dchannels, nprobe,
      axis.vmin, axis.dv, max_cells, drow);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, drow, sizeof(double) * nvalue,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

#endif /* CMI_RENDER_DRIVER_H */
