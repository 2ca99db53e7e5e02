/*
 * scatter_driver.h - the host side of the Monte Carlo scattered-light modes
 * (included from engine.hip): the dusty CCD image, the cell source, the sky
 * camera, several views per run, the scattered cubes, Lyman alpha and its
 * radiation field. A Monte Carlo call is
 *   - a setup: the engine's run-time choice (source, camera, cube on or off;
 *     for Lyman alpha the field on or off) mapped onto one instantiation of
 *     the kernel, with the camera argument built once per kind,
 *   - for a shoot, the chunk loop: launches sized from the steps per packet
 *     that the one before them took,
 *   - for a probe, the scaffold: rows up, launches of at most
 *     CMI_DUST_PROBE_LAUNCH rows, rows down,
 *   - for a setter, an arena (render_driver.h's) in which everything new is
 *     built aside and which the engine takes over only if nothing failed,
 * and the entry points are argument checks and one call into these.
 *
 * The header follows render_driver.h, which it takes RenderArena,
 * check_sigma_turb, check_have_cells, sky_map_check and line_cube_axis from;
 * dust_cube_mark_stale is declared ahead of both. dust_shoot_kernel,
 * dust_probe_kernel and lya_shoot_kernel are named inside the launcher
 * templates dust_launch_shoot, dust_launch_probe and lya_launch_shoot, which
 * generic lambdas in the entry points call: the rule of DESIGN_LOG.md 10 and
 * 15 - a template kernel first named in a function that is no template -
 * is not kept here, and the order of these kernels in the code object is
 * whatever the order of instantiation gives (behind the renderers' kernels).
 * What is held instead is each function's code, compared with the parent's
 * listing function by function (DESIGN_LOG.md 18).
 */
#ifndef CMI_SCATTER_DRIVER_H
#define CMI_SCATTER_DRIVER_H

/* dust_shoot_kernel launches: the first takes CMI_DUST_FIRST_LAUNCH
 * packets; every later one is sized from the DDA steps per packet measured so
 * far so that it takes about CMI_DUST_STEPS_PER_LAUNCH steps (~20 ms at the
 * measured 2.5e10 steps/s), between 64 and 2^20 packets. A dense medium, whose
 * packets scatter many times, thus gets short launches too. */
#define CMI_DUST_FIRST_LAUNCH (1ull << 14)
#define CMI_DUST_MIN_LAUNCH 64ull
#define CMI_DUST_MAX_LAUNCH (1ull << 20)
#define CMI_DUST_STEPS_PER_LAUNCH (1ull << 29)
/* With several views a packet takes K times the peel-off marches, and sized
 * by steps alone a launch soon holds fewer packets than the device has lanes
 * for (at K = 16 about 1e5 against 256 CUs x 512 lanes: measured at 0.6 of
 * the single camera's steps/s). Such a launch is no shorter
 * for being smaller - its lanes run side by side and it lasts as long as its
 * longest packets -, so these kinds are not sized below CMI_DUST_VIEWS_FILLS
 * times the lanes the device holds at once: CMI_DUST_VIEWS_LANES_PER_CU per
 * CU, 4 SIMDs x 2 waves (the kernels' 170 to 212 VGPRs) x 64 lanes. The
 * single camera's sizing is as it was. */
#define CMI_DUST_VIEWS_LANES_PER_CU 512ull
#define CMI_DUST_VIEWS_FILLS 4ull
/* rows per dust_probe_kernel or lya_probe_kernel launch */
#define CMI_DUST_PROBE_LAUNCH (1ll << 14)

/* packets of the first lya_shoot_kernel launch of a call; the later ones are
 * sized from its cell crossings per packet, as cmi_gpu_dust_shoot sizes its
 * own, between these bounds */
#define CMI_LYA_FIRST_LAUNCH (1ull << 14)
#define CMI_LYA_MIN_LAUNCH (1ull << 14)
#define CMI_LYA_MAX_LAUNCH (1ull << 20)
#define CMI_LYA_STEPS_PER_LAUNCH (1ull << 33)
/* workgroups per CU of the event loop (-DCMI_LYA_EVENT_LOOP; one packet per
 * lane launches a lane per packet): 8 x 4 waves wait for the 2 per SIMD that
 * the kernel's registers allow */
#define CMI_LYA_BLOCKS_PER_CU 8u
#define CMI_LYA_MAX_SCATTER 100000000u

/* ------------------------------------------------------- the cameras -- */

static bool dust_point_camera(const cmi_gpu_engine *e) {
  return e->dust_camera == DUST_CAMERA_POINT ||
         e->dust_camera == DUST_CAMERA_POINT_VIEWS;
}

static bool dust_several_views(const cmi_gpu_engine *e) {
  return e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS ||
         e->dust_camera == DUST_CAMERA_POINT_VIEWS;
}

/* pixels of one image of the selected camera */
static size_t dust_image_pixels(const cmi_gpu_engine *e) {
  return dust_point_camera(e)
             ? (size_t)e->sky_camera.nlon * e->sky_camera.nlat
             : (size_t)e->dust.res[0] * e->dust.res[1];
}

/* cube mode does not outlive what it was built from (the cameras, the cell
 * source, the velocities): the next shoot or probe fails until
 * cmi_gpu_set_scattered_cube is called again */
static void dust_cube_mark_stale(cmi_gpu_engine *e, const char *why) {
  if (e->dust_cube.nchan)
    e->dust_cube_stale = why;
  /* Lyman-alpha mode is built from the same things */
  if (e->lya.nchan)
    e->lya_stale = why;
}

/* the camera's part of DustDev, view by view */
static void dust_put_view(DustDev &d, const DustViewDev &v) {
  for (int j = 0; j < 5; ++j)
    d.view[j] = v.view[j];
  for (int a = 0; a < 3; ++a) {
    d.obs_dir[a] = v.obs_dir[a];
    d.obs_inv_dir[a] = v.obs_inv_dir[a];
  }
  for (int a = 0; a < 2; ++a) {
    d.img_anchor[a] = v.img_anchor[a];
    d.img_sides[a] = v.img_sides[a];
  }
}

/* the same for an observer of the point camera */
static void sky_put_observer(SkyCameraDev &cam, const SkyObserverDev &v) {
  for (int a = 0; a < 3; ++a) {
    cam.o[a] = v.o[a];
    cam.e1[a] = v.e1[a];
    cam.e2[a] = v.e2[a];
    cam.e3[a] = v.e3[a];
  }
  cam.r_min2 = v.r_min2;
  cam.pole_is_z = v.pole_is_z;
}

static SkyObserverDev sky_make_observer(const double *origin,
                                        const double *frame,
                                        double exclusion_radius) {
  SkyObserverDev v;
  for (int a = 0; a < 3; ++a) {
    v.o[a] = origin[a];
    v.e1[a] = frame[a];
    v.e2[a] = frame[3 + a];
    v.e3[a] = frame[6 + a];
  }
  v.r_min2 = exclusion_radius * exclusion_radius;
  v.pole_is_z = frame[6] == 0. && frame[7] == 0. && frame[8] == 1.;
  return v;
}

/* CCDImage ctor, src/CCDImage.hpp:123-160 */
static DustViewDev dust_make_view(double theta, double phi,
                                  const double *anchor, const double *sides) {
  DustViewDev v;
  v.view[0] = std::sin(theta);
  v.view[1] = std::cos(theta);
  v.view[2] = phi;
  v.view[3] = std::sin(phi);
  v.view[4] = std::cos(phi);
  v.obs_dir[0] = v.view[0] * v.view[4];
  v.obs_dir[1] = v.view[0] * v.view[3];
  v.obs_dir[2] = v.view[1];
  for (int a = 0; a < 3; ++a)
    v.obs_inv_dir[a] = 1. / v.obs_dir[a];
  for (int a = 0; a < 2; ++a) {
    v.img_anchor[a] = anchor[a];
    v.img_sides[a] = sides[a];
  }
  return v;
}

/* A camera replaces the selected one in two steps. The image stack and, with
 * several views (descriptors given), the descriptors and the per-view
 * counters are allocated before anything of the engine changes: a call that
 * fails here leaves the camera that was selected. Then the engine takes the
 * buffers over from the arena; the old image, descriptors and counters go. */
static int dust_new_camera(cmi_gpu_engine *e, const char *what, int32_t nviews,
                           size_t npixel, const void *descriptors,
                           size_t descriptor_bytes) {
  HIP_TRY(hipSetDevice(e->device));
  RenderArena arena;
  double *images = nullptr;
  char *views = nullptr;
  unsigned long long *counters = nullptr;
  int rc = arena.alloc(images, (size_t)nviews * 3 * npixel);
  if (!rc && descriptors)
    rc = arena.alloc(views, (size_t)nviews * descriptor_bytes);
  if (!rc && descriptors)
    rc = arena.alloc(counters, (size_t)nviews * CMI_DUST_VIEW_COUNTERS *
                                   CMI_DUST_VIEW_SLOTS);
  if (arena.out_of_memory)
    return fail(CMI_GPU_ENOMEM, "%s: the stack of %d images of %zu pixels "
                "does not fit into the device's memory", what, (int)nviews,
                npixel);
  CMI_TRY(rc);
  if (descriptors)
    HIP_TRY(hipMemcpy(views, descriptors, (size_t)nviews * descriptor_bytes,
                      hipMemcpyHostToDevice));
  HIP_TRY(hipStreamSynchronize(e->stream));
  /* no launch may see the old image once it is freed, whatever follows */
  e->have_ccd = false;
  (void)hipFree(e->dust_image);
  (void)hipFree(e->dust_views_dev);
  (void)hipFree(e->dust_view_counters);
  arena.release();
  e->dust_image = images;
  e->dust_views_dev = views;
  e->dust_view_counters = counters;
  e->dust_views.clear();
  e->sky_views.clear();
  e->dust_nviews = nviews;
  e->dust_probe_view = 0;
  return CMI_GPU_OK;
}

/* the parallel cameras: views[0] is the one DustDev holds; one view and no
 * several: the single camera and its kernels */
static int dust_set_parallel_cameras(cmi_gpu_engine *e, const char *what,
                                     const std::vector<DustViewDev> &views,
                                     bool several, int32_t nx, int32_t ny) {
  CMI_TRY(dust_new_camera(e, what, (int32_t)views.size(), (size_t)nx * ny,
                          several ? views.data() : nullptr,
                          sizeof(DustViewDev)));
  DustDev &d = e->dust;
  dust_put_view(d, views[0]);
  d.res[0] = nx;
  d.res[1] = ny;
  d.image = e->dust_image;
  if (several)
    e->dust_views = views;
  e->sky_camera.image = nullptr;
  e->dust_camera = several ? DUST_CAMERA_PARALLEL_VIEWS : DUST_CAMERA_PARALLEL;
  e->have_ccd = true;
  dust_cube_mark_stale(e, several ? "the cameras were set again"
                                  : "the camera was set again");
  return cmi_gpu_reset_image(e);
}

/* the point cameras: the window is shared, views[0] is the observer that
 * SkyCameraDev holds */
static int dust_set_point_cameras(cmi_gpu_engine *e, const char *what,
                                  const std::vector<SkyObserverDev> &views,
                                  bool several, double lon_min, double lon_max,
                                  double lat_min, double lat_max, int32_t nlon,
                                  int32_t nlat, int32_t direct_light) {
  CMI_TRY(dust_new_camera(e, what, (int32_t)views.size(), (size_t)nlon * nlat,
                          several ? views.data() : nullptr,
                          sizeof(SkyObserverDev)));
  SkyCameraDev cam = {};
  sky_put_observer(cam, views[0]);
  cam.lon_min = lon_min;
  cam.lat_min = lat_min;
  cam.lon_width = lon_max - lon_min;
  cam.lat_width = lat_max - lat_min;
  cam.nlon = nlon;
  cam.nlat = nlat;
  cam.direct_light = direct_light != 0;
  cam.image = e->dust_image;
  e->sky_camera = cam;
  if (several)
    e->sky_views = views;
  e->dust.image = nullptr;
  e->dust_camera = several ? DUST_CAMERA_POINT_VIEWS : DUST_CAMERA_POINT;
  e->have_ccd = true;
  dust_cube_mark_stale(e, several ? "the cameras were set again"
                                  : "the camera was set again");
  return cmi_gpu_reset_image(e);
}

/* ---------------------------------------------------------- the checks -- */

/* what the dust mode asks of the grid, for either source */
static int dust_check_grid(const cmi_gpu_engine *e) {
  const GridDev &g = e->grid;
  if (g.decomposed)
    return fail(CMI_GPU_ESTATE, "dust: not available on a block of a "
                                "decomposed grid");
  if (g.periodic[0] || g.periodic[1] || g.periodic[2])
    return fail(CMI_GPU_EINVAL,
                "dust: periodic boxes are not supported (the reference's "
                "integrate_optical_depth never reaches the edge of a periodic "
                "box, src/CartesianDensityGrid.cpp:187-227,341)");
  return CMI_GPU_OK;
}

static int check_camera_set(const cmi_gpu_engine *e, const char *what) {
  if (!e->have_ccd)
    return fail(CMI_GPU_ESTATE, "%s: a camera must be set first", what);
  return CMI_GPU_OK;
}

/* (hint: what the caller has to say about the sources) */
static int check_cell_source_selected(const cmi_gpu_engine *e,
                                      const char *what, const char *hint) {
  if (e->dust_source != DUST_SOURCE_CELLS || !e->have_cell_source)
    return fail(CMI_GPU_ESTATE, "%s: a cell source must be selected (%s)",
                what, hint);
  return CMI_GPU_OK;
}

/* a line source is of the cells it was set from */
static int check_cell_source_current(const cmi_gpu_engine *e,
                                     const char *what) {
  if (e->cell_source_from_cells && e->cell_source_epoch != e->cells_epoch)
    return fail(CMI_GPU_ESTATE, "%s: the cells changed after the line source "
                "was set; set_cell_source_line again", what);
  return CMI_GPU_OK;
}

static int check_view(const char *what, int32_t view, int32_t nviews) {
  if (view < 0 || view >= nviews)
    return fail(CMI_GPU_EINVAL, "%s: view %d of %d", what, (int)view,
                (int)nviews);
  return CMI_GPU_OK;
}

static int check_lya_mode(const cmi_gpu_engine *e, const char *what) {
  if (!e->lya.nchan)
    return fail(CMI_GPU_ESTATE, "%s: Lyman-alpha mode is not set "
                "(set_lyman_alpha)", what);
  return CMI_GPU_OK;
}

/* -------------------------------------- setup, chunk loop, scaffold -- */

extern "C++" {
namespace {
/* the kernel argument of the engine's camera as kind CAMERA: nothing for the
 * parallel camera, sky for the point camera, the descriptors, the stack and
 * the counters for the several views (with sky as what the observers share) */
template <int CAMERA>
DustCamera<CAMERA> scatter_camera(const cmi_gpu_engine *e,
                                  const SkyCameraDev &sky) {
  DustCamera<CAMERA> cam;
  if constexpr (CAMERA == DUST_CAMERA_POINT)
    cam = sky;
  if constexpr (CAMERA == DUST_CAMERA_POINT_VIEWS)
    cam.shared = sky;
  if constexpr (CAMERA == DUST_CAMERA_PARALLEL_VIEWS ||
                CAMERA == DUST_CAMERA_POINT_VIEWS) {
    cam.views = static_cast<decltype(cam.views)>(e->dust_views_dev);
    cam.nviews = e->dust_nviews;
    cam.images = e->dust_image;
    cam.counters = e->dust_view_counters;
  }
  return cam;
}

/* f(source, camera, cube) with the kernel arguments whose types select the
 * instantiation of a dust kernel: the several views' kinds or the single
 * cameras' (VIEWS), the point or the parallel one (the engine's), cube mode
 * (cube not null; the cell source then, as cmi_gpu_set_scattered_cube and
 * dust_prepare saw to), and the source (the engine's; the point cameras have
 * the cell source alone). Five instantiations per VIEWS, no other exists. */
template <bool VIEWS, class F>
void scatter_for_setup(const cmi_gpu_engine *e, const SkyCameraDev &sky,
                       const DustCubeDev *cube, F &&f) {
  constexpr int POINT = VIEWS ? DUST_CAMERA_POINT_VIEWS : DUST_CAMERA_POINT;
  constexpr int PARALLEL =
      VIEWS ? DUST_CAMERA_PARALLEL_VIEWS : DUST_CAMERA_PARALLEL;
  const DustCube<false> no_cube;
  const bool point = dust_point_camera(e);
  if (cube && point)
    f(e->cell_source, scatter_camera<POINT>(e, sky), *cube);
  else if (cube)
    f(e->cell_source, scatter_camera<PARALLEL>(e, sky), *cube);
  else if (point)
    f(e->cell_source, scatter_camera<POINT>(e, sky), no_cube);
  else if (e->dust_source == DUST_SOURCE_CELLS)
    f(e->cell_source, scatter_camera<PARALLEL>(e, sky), no_cube);
  else
    f(DustSource<DUST_SOURCE_GALAXY>(), scatter_camera<PARALLEL>(e, sky),
      no_cube);
}

/* packets [first, first + n) */
template <int SOURCE, int CAMERA, bool CUBE>
void dust_launch_shoot(cmi_gpu_engine *e, uint32_t seed, uint64_t first,
                       uint64_t n, const DustSource<SOURCE> &src,
                       const DustCamera<CAMERA> &cam,
                       const DustCube<CUBE> &cube) {
  dust_shoot_kernel<SOURCE, CAMERA, CUBE>
      <<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(
          e->grid, e->dust, e->dust_opacity, seed, first, n, e->dust_counters,
          src, cam, cube);
}

/* what a probe launch is given beyond the setup */
struct DustProbeRows {
  int32_t kind, width, max_events;
  uint32_t seed;
  uint64_t first;
  int64_t n;
  const double *in;
  double *out;
};

template <int SOURCE, int CAMERA, bool CUBE>
void dust_launch_probe(cmi_gpu_engine *e, const DustDev &dust,
                       const DustProbeRows &r, const DustSource<SOURCE> &src,
                       const DustCamera<CAMERA> &cam,
                       const DustCube<CUBE> &cube) {
  dust_probe_kernel<SOURCE, CAMERA, CUBE>
      <<<(unsigned)((r.n + 63) / 64), 64, 0, e->stream>>>(
          e->grid, dust, src, cam, cube, e->dust_opacity, r.kind, r.seed,
          r.first, r.n, r.width, r.in, r.out, r.max_events);
}

/* (field: LyaFieldDev or nothing) */
template <int CAMERA, class... FIELD>
void lya_launch_shoot(cmi_gpu_engine *e, const DustDev &dust, unsigned blocks,
                      uint32_t seed, uint64_t first, uint64_t n,
                      const DustCamera<CAMERA> &cam, const FIELD &...field) {
  lya_shoot_kernel<CAMERA, FIELD...><<<blocks, 256, 0, e->stream>>>(
      e->grid, dust, e->cell_source, cam, e->lya, seed, first, n, e->lya_next,
      e->lya_counters, field...);
}

/* one launch of chunk packets between the engine's timer events */
template <class F>
int scatter_timed_launch(cmi_gpu_engine *e, uint64_t chunk, F &&launch) {
  EventPair ev;
  CMI_TRY(timer_begin(e, ev));
  launch();
  HIP_TRY(hipGetLastError());
  return timer_end(e, e->shoot_events, ev, chunk);
}

/* The chunk loop of a shoot of n packets: the first launch takes `first`
 * packets; every later one is sized from the steps per packet of the one
 * before it (the device counter *nsteps, read before and after) so that it
 * takes about `steps` steps, between `min` and `max` packets.
 * enqueue(done, chunk) enqueues the launch of chunk packets after the first
 * done ones. */
struct ScatterChunks {
  uint64_t first, min, max, steps;
};

template <class F>
int scatter_chunk_loop(cmi_gpu_engine *e, const ScatterChunks &b,
                       const unsigned long long *nsteps, uint64_t n,
                       F &&enqueue) {
  uint64_t size = b.first;
  for (uint64_t done = 0; done < n;) {
    const uint64_t chunk = std::min<uint64_t>(n - done, size);
    /* only a launch that another follows is measured: both copies are
     * waited for below, before these variables end */
    const bool measure = done + chunk < n;
    unsigned long long steps_before = 0, steps_after = 0;
    if (measure)
      HIP_TRY(hipMemcpyAsync(&steps_before, nsteps, sizeof steps_before,
                             hipMemcpyDeviceToHost, e->stream));
    CMI_TRY(enqueue(done, chunk));
    done += chunk;
    if (measure) {
      /* the next launch's size from this one's steps per packet */
      HIP_TRY(hipMemcpyAsync(&steps_after, nsteps, sizeof steps_after,
                             hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      const double per_packet =
          std::max(1., (double)(steps_after - steps_before) / (double)chunk);
      size = (uint64_t)std::min<double>(
          (double)b.max,
          std::max<double>((double)b.min, (double)b.steps / per_packet));
    }
  }
  return CMI_GPU_OK;
}

/* The scaffold of a probe of n rows: in[n][in_width] (none with in_width 0)
 * goes up, out[n][width] comes down, and launch(rows_in, rows_out, first, m)
 * enqueues rows [first, first + m) - short launches: a row of a trace can be
 * a whole packet. */
template <class F>
int scatter_probe_rows(cmi_gpu_engine *e, int64_t n, int in_width, int width,
                       const double *in, double *out, F &&launch) {
  RenderArena arena;
  double *din = nullptr, *dout = nullptr;
  const size_t nout = (size_t)n * width;
  CMI_TRY(arena.alloc(dout, nout));
  if (in_width)
    CMI_TRY(arena.upload(din, in, (size_t)n * in_width));
  HIP_TRY(hipMemsetAsync(dout, 0, nout * sizeof(double), e->stream));
  for (int64_t k = 0; k < n; k += CMI_DUST_PROBE_LAUNCH) {
    const int64_t m = std::min<int64_t>(n - k, CMI_DUST_PROBE_LAUNCH);
    launch(din ? din + k * in_width : nullptr, dout + k * width, k, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  HIP_TRY(hipMemcpy(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}
} // namespace
} // extern "C++"

/* the plane [npixel][nchan] of a cube, the channel running fastest as the
 * kernels fill it, brought down as dst[nchan][npixel] through ordered */
static int scatter_download_plane(cmi_gpu_engine *e, const double *plane,
                                  int64_t npixel, int32_t nchan,
                                  double *ordered, double *dst) {
  const size_t nvalue = (size_t)npixel * nchan;
  dust_cube_reorder_kernel<<<(unsigned)((nvalue + 255) / 256), 256, 0,
                             e->stream>>>(plane, npixel, nchan, ordered);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(dst, ordered, sizeof(double) * nvalue,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

/* the device's counters of the dust modes once the stream is idle (zeros
 * before the first launch) */
static int dust_read_counters(cmi_gpu_engine *e, DustCountersDev &c) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  c = DustCountersDev{};
  if (e->dust_counters)
    HIP_TRY(hipMemcpy(&c, e->dust_counters, sizeof c, hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

/* what set_scattered_cube and set_lyman_alpha answer when a build failed: rc
 * is the failure, and running out of device memory has a message of its own */
static int scatter_build_failed(const char *what, int rc, bool out_of_memory,
                                int32_t nviews, int32_t nchan, size_t npixel) {
  if (out_of_memory)
    return fail(CMI_GPU_ENOMEM, "%s: %d cubes of %d channels of %zu pixels do "
                "not fit into the device's memory", what, (int)nviews,
                (int)nchan, npixel);
  return rc;
}

/* ------------------------------------------ dusty radiative transfer -- */

int cmi_gpu_set_dust_scattering(cmi_gpu_engine *e, double g, double p_l,
                                double albedo, double kappa) {
  if (!e || !(g != 0.) || !(kappa >= 0.))
    return fail(CMI_GPU_EINVAL, "set_dust_scattering: bad argument (g must "
                                "be non-zero, kappa >= 0)");
  /* DustScattering ctor, src/DustScattering.hpp:171-185 */
  DustDev &d = e->dust;
  d.hgg = g;
  d.g2 = g * g;
  d.omg2 = 1. - d.g2;
  d.thgg = 2. * g;
  d.omhgg = 1. - g;
  d.od2hgg = 0.5 / g;
  d.opg2 = 1. + d.g2;
  d.pl = p_l;
  d.sc = 1.;
  d.pc = 0.;
  d.albedo = albedo;
  e->dust_kappa = kappa;
  e->dust_per_hydrogen = false;
  e->have_dust_scattering = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_dust_scattering_per_hydrogen(cmi_gpu_engine *e, double g,
                                             double p_l, double albedo,
                                             double sigma) {
  if (!e || !(sigma >= 0.) || !std::isfinite(sigma))
    return fail(CMI_GPU_EINVAL, "set_dust_scattering_per_hydrogen: bad "
                                "argument (sigma must be >= 0)");
  /* the same phase function constants; kappa 0 passes its check */
  CMI_TRY(cmi_gpu_set_dust_scattering(e, g, p_l, albedo, 0.));
  e->dust_kappa = sigma;
  e->dust_per_hydrogen = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_ccd_image(cmi_gpu_engine *e, double theta, double phi,
                          int32_t nx, int32_t ny, const double *anchor,
                          const double *sides) {
  if (!e || nx <= 0 || ny <= 0 || !anchor || !sides || !(sides[0] > 0.) ||
      !(sides[1] > 0.) || (int64_t)nx * ny > (1ll << 28))
    return fail(CMI_GPU_EINVAL, "set_ccd_image: bad argument");
  return dust_set_parallel_cameras(
      e, "set_ccd_image", {dust_make_view(theta, phi, anchor, sides)}, false,
      nx, ny);
}

int cmi_gpu_set_ccd_images(cmi_gpu_engine *e, int32_t nviews,
                           const double *theta, const double *phi, int32_t nx,
                           int32_t ny, const double *anchors,
                           const double *sides) {
  if (!e || !theta || !phi || !anchors || !sides || nx <= 0 || ny <= 0 ||
      (int64_t)nx * ny > (1ll << 28))
    return fail(CMI_GPU_EINVAL, "set_ccd_images: bad argument");
  if (nviews < 1 || nviews > CMI_GPU_MAX_VIEWS)
    return fail(CMI_GPU_EINVAL, "set_ccd_images: %d views, must be 1 to %d",
                (int)nviews, CMI_GPU_MAX_VIEWS);
  std::vector<DustViewDev> views;
  for (int32_t v = 0; v < nviews; ++v) {
    if (!(sides[2 * v] > 0.) || !(sides[2 * v + 1] > 0.))
      return fail(CMI_GPU_EINVAL, "set_ccd_images: view %d: bad argument (the "
                  "sides must be > 0)", (int)v);
    views.push_back(
        dust_make_view(theta[v], phi[v], anchors + 2 * v, sides + 2 * v));
  }
  return dust_set_parallel_cameras(e, "set_ccd_images", views, true, nx, ny);
}

int cmi_gpu_check_sky_camera(const double *box_anchor, const double *box_sides,
                             const double *origin, const double *frame,
                             double lon_min, double lon_max, double lat_min,
                             double lat_max, int32_t nlon, int32_t nlat,
                             double exclusion_radius) {
  static const char *what = "set_sky_camera";
  if (!box_anchor || !box_sides || !origin)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(origin[a]))
      return fail(CMI_GPU_EINVAL, "%s: the origin is not finite", what);
  CMI_TRY(sky_map_check(what, frame, lon_min, lon_max, lat_min, lat_max, nlon,
                        nlat));
  /* (a Monte Carlo event must land in one pixel: no more than one turn) */
  if (!(lon_max <= lon_min + 2. * M_PI))
    return fail(CMI_GPU_EINVAL, "%s: the longitude range must not be wider "
                "than 2 pi", what);
  if (!(exclusion_radius >= 0.) || !std::isfinite(exclusion_radius))
    return fail(CMI_GPU_EINVAL, "%s: the exclusion radius must be finite and "
                ">= 0", what);
  bool in_box = true;
  for (int a = 0; a < 3; ++a)
    in_box &= origin[a] >= box_anchor[a] &&
              origin[a] <= box_anchor[a] + box_sides[a];
  if (in_box && !(exclusion_radius > 0.))
    return fail(CMI_GPU_EINVAL, "%s: an observer in the box needs an "
                "exclusion radius above 0 (the estimator's 1 / r^2 diverges "
                "at the observer)", what);
  return CMI_GPU_OK;
}

int cmi_gpu_set_sky_camera(cmi_gpu_engine *e, const double *origin,
                           const double *frame, double lon_min, double lon_max,
                           double lat_min, double lat_max, int32_t nlon,
                           int32_t nlat, double exclusion_radius,
                           int32_t direct_light) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "set_sky_camera: null engine");
  CMI_TRY(cmi_gpu_check_sky_camera(e->grid.anchor, e->grid.box_sides, origin,
                                   frame, lon_min, lon_max, lat_min, lat_max,
                                   nlon, nlat, exclusion_radius));
  return dust_set_point_cameras(
      e, "set_sky_camera",
      {sky_make_observer(origin, frame, exclusion_radius)}, false, lon_min,
      lon_max, lat_min, lat_max, nlon, nlat, direct_light);
}

int cmi_gpu_set_sky_cameras(cmi_gpu_engine *e, int32_t nviews,
                            const double *origins, const double *frames,
                            double lon_min, double lon_max, double lat_min,
                            double lat_max, int32_t nlon, int32_t nlat,
                            const double *exclusion_radii,
                            int32_t direct_light) {
  if (!e || !origins || !frames || !exclusion_radii)
    return fail(CMI_GPU_EINVAL, "set_sky_cameras: null argument");
  if (nviews < 1 || nviews > CMI_GPU_MAX_VIEWS)
    return fail(CMI_GPU_EINVAL, "set_sky_cameras: %d views, must be 1 to %d",
                (int)nviews, CMI_GPU_MAX_VIEWS);
  std::vector<SkyObserverDev> views;
  for (int32_t v = 0; v < nviews; ++v) {
    if (cmi_gpu_check_sky_camera(e->grid.anchor, e->grid.box_sides,
                                 origins + 3 * v, frames + 9 * v, lon_min,
                                 lon_max, lat_min, lat_max, nlon, nlat,
                                 exclusion_radii[v])) {
      /* set_sky_camera's message, with the view it is about */
      const std::string single = g_last_error;
      return fail(CMI_GPU_EINVAL, "set_sky_cameras: view %d: %s", (int)v,
                  single.c_str());
    }
    views.push_back(sky_make_observer(origins + 3 * v, frames + 9 * v,
                                      exclusion_radii[v]));
  }
  return dust_set_point_cameras(e, "set_sky_cameras", views, true, lon_min,
                                lon_max, lat_min, lat_max, nlon, nlat,
                                direct_light);
}

int cmi_gpu_set_continuous_source_spiral_galaxy(cmi_gpu_engine *e,
                                                double r_stars, double h_stars,
                                                double bulge_over_total) {
  if (!e || !(r_stars > 0.) || !(h_stars > 0.))
    return fail(CMI_GPU_EINVAL,
                "set_continuous_source_spiral_galaxy: bad argument");
  /* the sampler assumes a box centred on the origin
   * (src/SpiralGalaxyContinuousPhotonSource.hpp:112-113): its rejection loop
   * would practically never end for a box away from the galaxy */
  for (int a = 0; a < 3; ++a)
    if (!(0. >= e->grid.anchor[a] &&
          0. < e->grid.anchor[a] + e->grid.box_sides[a]))
      return fail(CMI_GPU_EINVAL,
                  "set_continuous_source_spiral_galaxy: the box must contain "
                  "the origin (the galaxy's centre)");
  HIP_TRY(hipSetDevice(e->device));
  /* SpiralGalaxyContinuousPhotonSource ctor,
   * src/SpiralGalaxyContinuousPhotonSource.hpp:98-150 */
  DustDev &d = e->dust;
  const double kpc = 3.086e19;
  d.rC = 0.2 * kpc;
  d.rB = 2. * kpc;
  d.rJ = 0.4 * kpc;
  d.r_stars = r_stars;
  d.h_stars = h_stars;
  d.rB_over_rJ_plus_rB = d.rB / (d.rB + d.rJ);
  d.rC_over_rJ_plus_rC = d.rC / (d.rC + d.rJ);
  d.bulge_to_total =
      bulge_over_total * (1. - d.rC_over_rJ_plus_rC / d.rB_over_rJ_plus_rB);
  for (int a = 0; a < 3; ++a) {
    d.box_anchor[a] = e->grid.anchor[a];
    d.box_sides[a] = e->grid.box_sides[a];
  }
  const double *A = d.box_anchor;
  const double rmax = 1.2 * std::sqrt(A[0] * A[0] + A[1] * A[1] + A[2] * A[2]);
  const int nbin = 1000;
  std::vector<double> cdf(2 * (nbin + 1));
  for (int i = 0; i < nbin; ++i) {
    const double w = i * rmax / nbin;
    const double x = w / r_stars;
    cdf[i] = w;
    cdf[nbin + 1 + i] = 1. - (1. + x) * std::exp(-x);
  }
  cdf[nbin] = rmax;
  cdf[2 * nbin + 1] = 1.;
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (!e->dust_cdf)
    HIP_TRY(hipMalloc(&e->dust_cdf, cdf.size() * sizeof(double)));
  HIP_TRY(hipMemcpy(e->dust_cdf, cdf.data(), cdf.size() * sizeof(double),
                    hipMemcpyHostToDevice));
  d.cdf_x = e->dust_cdf;
  d.cdf_y = e->dust_cdf + nbin + 1;
  d.cdf_n = nbin + 1;
  e->have_dust_source = true;
  e->dust_source = DUST_SOURCE_GALAXY;
  dust_cube_mark_stale(e, "the source was replaced");
  return CMI_GPU_OK;
}

/* the cell source's tables from the weights in e->cell_source_cells (device_
 * dust.h has the contract): refuses bad weights and a source that does not
 * emit, selects the source */
static int cell_source_build(cmi_gpu_engine *e, const char *what,
                             bool from_cells) {
  const int64_t ncell = e->ncell;
  const int64_t nblock =
      (ncell + CMI_CELL_SOURCE_BLOCK - 1) / CMI_CELL_SOURCE_BLOCK;
  if (!e->cell_source_blocks)
    HIP_TRY(hipMalloc(&e->cell_source_blocks, (size_t)nblock * sizeof(double)));
  RenderArena arena;
  unsigned int *ninvalid = nullptr;
  CMI_TRY(arena.alloc(ninvalid, 1));
  unsigned int bad = 0;
  std::vector<double> &B = e->cell_source_blocks_host;
  B.assign((size_t)nblock, 0.);
  HIP_TRY(hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream));
  cell_source_check_kernel<<<grid_blocks(e, ncell, 8), 256, 0, e->stream>>>(
      e->cell_source_cells, ncell, ninvalid);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (bad)
    return fail(CMI_GPU_EINVAL, "%s: %u weight(s) are negative or not finite",
                what, bad);
  cell_source_block_kernel<<<(unsigned)((nblock + 63) / 64), 64, 0,
                             e->stream>>>(e->cell_source_cells, ncell, nblock,
                                          e->cell_source_blocks);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(B.data(), e->cell_source_blocks,
                         (size_t)nblock * sizeof(double),
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  /* B: the running sum of the block totals, block by block */
  double total = 0.;
  for (int64_t b = 0; b < nblock; ++b) {
    total += B[(size_t)b];
    B[(size_t)b] = total;
  }
  if (!(total > 0.))
    return fail(CMI_GPU_ESTATE, "%s: nothing emits (the weights sum to 0)",
                what);
  if (!std::isfinite(total))
    return fail(CMI_GPU_EINVAL, "%s: the weights' sum is not finite", what);
  HIP_TRY(hipMemcpy(e->cell_source_blocks, B.data(),
                    (size_t)nblock * sizeof(double), hipMemcpyHostToDevice));
  e->cell_source.block_sums = e->cell_source_blocks;
  e->cell_source.cell_sums = e->cell_source_cells;
  e->cell_source.ncell = ncell;
  e->cell_source.nblock = nblock;
  e->cell_source_from_cells = from_cells;
  e->cell_source_epoch = e->cells_epoch;
  e->have_cell_source = true;
  e->dust_source = DUST_SOURCE_CELLS;
  return CMI_GPU_OK;
}

/* the checks both setters share; the weights' buffer */
static int cell_source_begin(cmi_gpu_engine *e) {
  CMI_TRY(dust_check_grid(e));
  HIP_TRY(hipSetDevice(e->device));
  /* no launch reads the tables while they are rebuilt; a failed build
   * leaves no source */
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->have_cell_source = false;
  dust_cube_mark_stale(e, "the cell source was replaced");
  if (!e->cell_source_cells)
    HIP_TRY(hipMalloc(&e->cell_source_cells,
                      (size_t)e->ncell * sizeof(double)));
  return CMI_GPU_OK;
}

int cmi_gpu_set_cell_source_line(cmi_gpu_engine *e, int32_t line) {
  static const char *what = "set_cell_source_line";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  if (line < 0 || line >= CMI_NEMISSIONLINE)
    return fail(CMI_GPU_EINVAL, "%s: no emission line %d", what, (int)line);
  CMI_TRY(check_have_cells(e, what));
  CMI_TRY(cell_source_begin(e));
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  CellSourceLineArgs a;
  a.model = e->model;
  a.cells = *cells;
  a.ncell = e->ncell;
  a.line = line;
  a.weights = e->cell_source_cells;
  cell_source_line_kernel<<<grid_blocks(e, e->ncell, 8), CMI_BLOCK, 0,
                            e->stream>>>(a);
  HIP_TRY(hipGetLastError());
  e->cell_source_line = line;
  return cell_source_build(e, what, true);
}

int cmi_gpu_set_cell_source_field(cmi_gpu_engine *e, const double *field) {
  static const char *what = "set_cell_source_field";
  if (!e || !field)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(cell_source_begin(e));
  HIP_TRY(hipMemcpy(e->cell_source_cells, field,
                    (size_t)e->ncell * sizeof(double), hipMemcpyHostToDevice));
  return cell_source_build(e, what, false);
}

int cmi_gpu_get_cell_source(cmi_gpu_engine *e, double *total_luminosity,
                            double *block_sums, double *cell_sums) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "get_cell_source: null engine");
  if (!e->have_cell_source)
    return fail(CMI_GPU_ESTATE, "get_cell_source: no cell source is set");
  const std::vector<double> &B = e->cell_source_blocks_host;
  if (total_luminosity)
    *total_luminosity = e->grid.cellside[0] * e->grid.cellside[1] *
                        e->grid.cellside[2] * B.back();
  if (block_sums)
    std::copy(B.begin(), B.end(), block_sums);
  if (cell_sums) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(cell_sums, e->cell_source_cells,
                      (size_t)e->ncell * sizeof(double),
                      hipMemcpyDeviceToHost));
  }
  return CMI_GPU_OK;
}

/* everything a dust launch needs; builds the records {n kappa x_H, 0} or
 * {n sigma, 0} */
static int dust_prepare(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  CMI_TRY(dust_check_grid(e));
  const bool have_source = e->dust_source == DUST_SOURCE_CELLS
                               ? e->have_cell_source
                               : e->have_dust_source;
  if (!e->have_cells || !e->have_dust_scattering || !e->have_ccd ||
      !have_source)
    return fail(CMI_GPU_ESTATE, "dust: upload_cells, set_dust_scattering, "
                                "a camera (set_ccd_image, set_sky_camera or "
                                "their several views) and "
                                "set_continuous_source_spiral_galaxy (or a "
                                "cell source) first");
  if (dust_point_camera(e) && e->dust_source != DUST_SOURCE_CELLS)
    return fail(CMI_GPU_ESTATE, "dust: the sky camera serves the cell source "
                                "only, not the spiral galaxy");
  if (e->dust_source == DUST_SOURCE_CELLS)
    CMI_TRY(check_cell_source_current(e, "dust"));
  if (e->dust_cube.nchan && e->dust_cube_stale)
    return fail(CMI_GPU_ESTATE, "dust: %s after cube mode was set; "
                "set_scattered_cube again", e->dust_cube_stale);
  HIP_TRY(hipSetDevice(e->device));
  if (!e->dust_opacity)
    HIP_TRY(hipMalloc(&e->dust_opacity, (size_t)e->ncell * sizeof(double2)));
  if (!e->dust_counters) {
    HIP_TRY(hipMalloc(&e->dust_counters, sizeof(DustCountersDev)));
    HIP_TRY(hipMemsetAsync(e->dust_counters, 0, sizeof(DustCountersDev),
                           e->stream));
  }
  const unsigned blocks = (unsigned)((e->ncell + 255) / 256);
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  if (e->dust_per_hydrogen)
    dust_opacity_per_hydrogen_kernel<<<blocks, 256, 0, e->stream>>>(
        cells->number_density, e->dust_kappa, e->ncell, e->dust_opacity);
  else
    dust_opacity_kernel<<<blocks, 256, 0, e->stream>>>(
        cells->number_density, cells->x[0], e->dust_kappa, e->ncell,
        e->dust_opacity);
  HIP_TRY(hipGetLastError());
  return CMI_GPU_OK;
}

int cmi_gpu_dust_shoot(cmi_gpu_engine *e, uint32_t seed, uint64_t first_packet,
                       uint64_t n) {
  CMI_TRY(dust_prepare(e));
  const bool several = dust_several_views(e);
  ScatterChunks bounds = {CMI_DUST_FIRST_LAUNCH, CMI_DUST_MIN_LAUNCH,
                          CMI_DUST_MAX_LAUNCH, CMI_DUST_STEPS_PER_LAUNCH};
  if (several)
    bounds.min = std::max<uint64_t>(CMI_DUST_MIN_LAUNCH,
                                    CMI_DUST_VIEWS_FILLS *
                                        (uint64_t)e->num_cu *
                                        CMI_DUST_VIEWS_LANES_PER_CU);
  const DustCubeDev *cube = e->dust_cube.nchan ? &e->dust_cube : nullptr;
  return scatter_chunk_loop(
      e, bounds, &e->dust_counters->nsteps, n,
      [&](uint64_t done, uint64_t chunk) {
        return scatter_timed_launch(e, chunk, [&] {
          auto launch = [&](const auto &src, const auto &cam, const auto &cb) {
            dust_launch_shoot(e, seed, first_packet + done, chunk, src, cam,
                              cb);
          };
          if (several)
            scatter_for_setup<true>(e, e->sky_camera, cube, launch);
          else
            scatter_for_setup<false>(e, e->sky_camera, cube, launch);
        });
      });
}

int cmi_gpu_get_dust_counters(cmi_gpu_engine *e, uint64_t *counters) {
  if (!e || !counters)
    return fail(CMI_GPU_EINVAL, "get_dust_counters: bad argument");
  DustCountersDev c;
  CMI_TRY(dust_read_counters(e, c));
  counters[0] = c.nsteps;
  counters[1] = c.nscatter;
  counters[2] = c.ncapped;
  counters[3] = c.natomics;
  counters[4] = c.npackets;
  counters[5] = c.nsource_capped;
  return CMI_GPU_OK;
}

int cmi_gpu_get_sky_camera_counters(cmi_gpu_engine *e, uint64_t *counters) {
  if (!e || !counters)
    return fail(CMI_GPU_EINVAL, "get_sky_camera_counters: bad argument");
  DustCountersDev c;
  CMI_TRY(dust_read_counters(e, c));
  counters[0] = c.nexcluded;
  counters[1] = c.noutside;
  return CMI_GPU_OK;
}

int cmi_gpu_download_image(cmi_gpu_engine *e, double *I, double *Q,
                           double *U) {
  return cmi_gpu_download_image_view(e, 0, I, Q, U);
}

int cmi_gpu_download_image_view(cmi_gpu_engine *e, int32_t view, double *I,
                                double *Q, double *U) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (!e->have_ccd)
    return fail(CMI_GPU_ESTATE, "download_image: no image (set_ccd_image or "
                                "set_sky_camera)");
  uint64_t c[6];
  CMI_TRY(cmi_gpu_get_dust_counters(e, c));
  if (c[5])
    return fail(CMI_GPU_ESTATE,
                "download_image: the source found no position in the box for "
                "%llu packet(s) in %u attempts; the image is incomplete",
                (unsigned long long)c[5], CMI_DUST_MAX_ATTEMPTS);
  if (c[2])
    return fail(CMI_GPU_ESTATE,
                "download_image: %llu packet(s) reached the cap of %d "
                "scatterings; the image is incomplete",
                (unsigned long long)c[2], CMI_DUST_MAX_SCATTER);
  CMI_TRY(check_view("download_image_view", view, e->dust_nviews));
  const size_t npixel = dust_image_pixels(e);
  double *dst[3] = {I, Q, U};
  for (int k = 0; k < 3; ++k)
    if (dst[k])
      HIP_TRY(hipMemcpy(dst[k], e->dust_image + (3 * (size_t)view + k) * npixel,
                        npixel * sizeof(double), hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

int cmi_gpu_reset_image(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (e->dust_image)
    HIP_TRY(hipMemsetAsync(e->dust_image, 0,
                           (size_t)e->dust_nviews * 3 * dust_image_pixels(e) *
                               sizeof(double),
                           e->stream));
  if (e->dust_view_counters)
    HIP_TRY(hipMemsetAsync(e->dust_view_counters, 0,
                           (size_t)e->dust_nviews * CMI_DUST_VIEW_COUNTERS *
                               CMI_DUST_VIEW_SLOTS *
                               sizeof(unsigned long long),
                           e->stream));
  if (e->dust_cube.nchan)
    HIP_TRY(hipMemsetAsync(e->dust_cube.cube, 0,
                           (size_t)e->dust_cube_nviews * 3 *
                               (size_t)e->dust_cube.npixel *
                               e->dust_cube.nchan * sizeof(double),
                           e->stream));
  if (e->dust_counters)
    HIP_TRY(hipMemsetAsync(e->dust_counters, 0, sizeof(DustCountersDev),
                           e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

int cmi_gpu_get_dust_view_counters(cmi_gpu_engine *e, int32_t view,
                                   uint64_t *counters) {
  if (!e || !counters)
    return fail(CMI_GPU_EINVAL, "get_dust_view_counters: bad argument");
  if (!e->have_ccd || !dust_several_views(e))
    return fail(CMI_GPU_ESTATE, "get_dust_view_counters: no camera with "
                                "several views is selected (set_ccd_images "
                                "or set_sky_cameras)");
  CMI_TRY(check_view("get_dust_view_counters", view, e->dust_nviews));
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  unsigned long long slots[CMI_DUST_VIEW_COUNTERS][CMI_DUST_VIEW_SLOTS];
  HIP_TRY(hipMemcpy(slots,
                    e->dust_view_counters + (size_t)view *
                                                CMI_DUST_VIEW_COUNTERS *
                                                CMI_DUST_VIEW_SLOTS,
                    sizeof slots, hipMemcpyDeviceToHost));
  for (int j = 0; j < CMI_DUST_VIEW_COUNTERS; ++j) {
    counters[j] = 0;
    for (int k = 0; k < CMI_DUST_VIEW_SLOTS; ++k)
      counters[j] += slots[j][k];
  }
  return CMI_GPU_OK;
}

int cmi_gpu_select_probe_view(cmi_gpu_engine *e, int32_t view) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (!e->have_ccd)
    return fail(CMI_GPU_ESTATE, "select_probe_view: no camera is set");
  CMI_TRY(check_view("select_probe_view", view, e->dust_nviews));
  e->dust_probe_view = view;
  return CMI_GPU_OK;
}

int cmi_gpu_dust_probe(cmi_gpu_engine *e, int32_t kind, uint32_t seed,
                       uint64_t first_packet, int64_t n, const double *in,
                       double *out, int32_t max_events) {
  if (!e || n < 0 || !out || kind < 0 || kind > DUST_PROBE_CUBE_TRACE ||
      max_events < 0 || n > (1 << 24))
    return fail(CMI_GPU_EINVAL, "dust_probe: bad argument");
  static const int in_width[8] = {0, 12, 12, 6, 0, 0, 15, 0};
  const int width = kind == DUST_PROBE_EMIT              ? 6
                    : kind == DUST_PROBE_SCATTER         ? 12
                    : kind == DUST_PROBE_SCATTER_TOWARDS ? 5
                    : kind == DUST_PROBE_OPTICAL_DEPTH   ? 2 + max_events
                    : kind == DUST_PROBE_CELL_SOURCE     ? 7
                    : kind == DUST_PROBE_SKY_PEEL        ? 9
                    : kind == DUST_PROBE_CUBE_TRACE      ? 4 + 10 * max_events
                                                         : 4 + 8 * max_events;
  if (in_width[kind] && !in)
    return fail(CMI_GPU_EINVAL, "dust_probe: input rows missing");
  CMI_TRY(dust_prepare(e));
  if (kind == DUST_PROBE_CELL_SOURCE && e->dust_source != DUST_SOURCE_CELLS)
    return fail(CMI_GPU_ESTATE, "dust_probe: no cell source is selected");
  if (kind == DUST_PROBE_SKY_PEEL && !dust_point_camera(e))
    return fail(CMI_GPU_ESTATE, "dust_probe: no sky camera is selected");
  if (kind == DUST_PROBE_CUBE_TRACE && !e->dust_cube.nchan)
    return fail(CMI_GPU_ESTATE, "dust_probe: cube mode is not set "
                                "(set_scattered_cube)");
  /* the selected view's observer velocity goes with its camera */
  DustCubeDev cube = e->dust_cube;
  if (cube.nchan)
    cube.obs_velocity += 3 * (size_t)e->dust_probe_view;
  /* with several views the probes run the single camera's kernels for the
   * selected view, so a row is the single camera's row (a trace writes to no
   * image) */
  DustDev dust = e->dust;
  SkyCameraDev sky_camera = e->sky_camera;
  if (e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS)
    dust_put_view(dust, e->dust_views[e->dust_probe_view]);
  if (e->dust_camera == DUST_CAMERA_POINT_VIEWS)
    sky_put_observer(sky_camera, e->sky_views[e->dust_probe_view]);
  if (n == 0)
    return CMI_GPU_OK;
  return scatter_probe_rows(
      e, n, in_width[kind], width, in, out,
      [&](const double *rows_in, double *rows_out, int64_t first, int64_t m) {
        const DustProbeRows r = {kind, width, max_events, seed,
                                 first_packet + first, m, rows_in, rows_out};
        scatter_for_setup<false>(
            e, sky_camera, kind == DUST_PROBE_CUBE_TRACE ? &cube : nullptr,
            [&](const auto &src, const auto &cam, const auto &cb) {
              dust_launch_probe(e, dust, r, src, cam, cb);
            });
      });
}

/* --------------------------------------- scattered-light line cubes -- */

static void dust_cube_free(cmi_gpu_engine *e) {
  (void)hipFree(const_cast<double *>(e->dust_cube.s2));
  (void)hipFree(const_cast<double *>(e->dust_cube.obs_velocity));
  (void)hipFree(e->dust_cube.cube);
  e->dust_cube = DustCubeDev{};
  e->dust_cube_nviews = 0;
  e->dust_cube_stale = nullptr;
}

/* the new cube's device memory in `kept`: the cells' variances from the line
 * source's temperatures or from the caller's widths, the observers'
 * velocities, the cubes */
static int dust_cube_build(cmi_gpu_engine *e, const char *what,
                           RenderArena &kept, RenderArena &scratch,
                           const CellsDev *cells, double sigma_turb,
                           const double *widths,
                           const std::vector<double> &vo, size_t ncube,
                           double *&s2, double *&vobs, double *&cube) {
  const size_t ncell = (size_t)e->ncell;
  CMI_TRY(kept.alloc(s2, ncell));
  CMI_TRY(kept.alloc(vobs, vo.size()));
  CMI_TRY(kept.alloc(cube, ncube));
  HIP_TRY(hipMemcpy(vobs, vo.data(), sizeof(double) * vo.size(),
                    hipMemcpyHostToDevice));
  unsigned int bad = 0;
  if (!widths) {
    dust_cube_line_variance_kernel<<<(unsigned)((ncell + 255) / 256), 256, 0,
                                     e->stream>>>(
        cells->temperature, cmi_emission_atomic_weight[e->cell_source_line],
        sigma_turb, e->ncell, s2);
    HIP_TRY(hipGetLastError());
  } else {
    double *dwidths = nullptr;
    unsigned int *ninvalid = nullptr;
    CMI_TRY(scratch.alloc(dwidths, ncell));
    CMI_TRY(scratch.alloc(ninvalid, 1));
    HIP_TRY(hipMemcpy(dwidths, widths, sizeof(double) * ncell,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream));
    dust_cube_field_variance_kernel<<<grid_blocks(e, e->ncell, 8), 256, 0,
                                      e->stream>>>(dwidths, e->ncell, s2,
                                                   ninvalid);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                           e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (bad)
    return fail(CMI_GPU_EINVAL, "%s: %u width(s) are negative or not finite",
                what, bad);
  return CMI_GPU_OK;
}

int cmi_gpu_set_scattered_cube(cmi_gpu_engine *e, int32_t nchan, double vmin,
                               double vmax, double sigma_turb,
                               const double *widths,
                               const double *observer_velocities) {
  static const char *what = "set_scattered_cube";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  HIP_TRY(hipSetDevice(e->device));
  if (nchan == 0) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    dust_cube_free(e);
    return CMI_GPU_OK;
  }
  CMI_TRY(check_camera_set(e, what));
  CMI_TRY(check_cell_source_selected(e, what,
                                     "the spiral galaxy has no line"));
  const bool line = e->cell_source_from_cells;
  CMI_TRY(check_cell_source_current(e, what));
  if (line && widths)
    return fail(CMI_GPU_ESTATE, "%s: a line source takes its widths from the "
                "cells' temperatures; widths must be NULL", what);
  if (!line && !widths)
    return fail(CMI_GPU_ESTATE, "%s: a field source needs widths[ncell]",
                what);
  if (line && cmi_emission_atomic_weight[e->cell_source_line] == 0.)
    return fail(CMI_GPU_EINVAL, "%s: entry %d is not the line of one ion: it "
                "has no line profile", what, (int)e->cell_source_line);
  CMI_TRY(check_sigma_turb(what, sigma_turb));
  const int32_t nviews = e->dust_nviews;
  if (observer_velocities)
    for (int32_t i = 0; i < 3 * nviews; ++i)
      if (!std::isfinite(observer_velocities[i]))
        return fail(CMI_GPU_EINVAL, "%s: the velocity of observer %d is not "
                    "finite", what, (int)(i / 3));
  const bool point = dust_point_camera(e);
  LineCubeAxis axis;
  CMI_TRY(line_cube_axis(what, nviews,
                         point ? e->sky_camera.nlon : e->dust.res[0],
                         point ? e->sky_camera.nlat : e->dust.res[1], nchan,
                         vmin, vmax, axis));
  const size_t npixel = dust_image_pixels(e);
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  std::vector<double> vo(3 * (size_t)nviews, 0.);
  if (observer_velocities)
    std::copy(observer_velocities, observer_velocities + vo.size(),
              vo.begin());
  /* everything new is built aside: a call that fails leaves the previous
   * state in place */
  RenderArena kept, scratch;
  double *s2 = nullptr, *vobs = nullptr, *cube = nullptr;
  const int rc = dust_cube_build(e, what, kept, scratch, cells, sigma_turb,
                                 widths, vo, 3 * (size_t)nviews * npixel * nchan,
                                 s2, vobs, cube);
  if (rc)
    return scatter_build_failed(what, rc,
                                kept.out_of_memory || scratch.out_of_memory,
                                nviews, nchan, npixel);
  dust_cube_free(e);
  kept.release();
  DustCubeDev &c = e->dust_cube;
  c.velocity = e->cell_velocities;
  c.ncell = e->ncell;
  c.s2 = s2;
  c.obs_velocity = vobs;
  c.two_sigma2 = 2. * sigma_turb * sigma_turb;
  c.nchan = nchan;
  c.vmin = axis.vmin;
  c.dv = axis.dv;
  c.npixel = (int64_t)npixel;
  c.cube = cube;
  e->dust_cube_nviews = nviews;
  return cmi_gpu_reset_image(e);
}

int cmi_gpu_download_cube_view(cmi_gpu_engine *e, int32_t view, double *I,
                               double *Q, double *U) {
  static const char *what = "download_cube_view";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  if (!e->dust_cube.nchan)
    return fail(CMI_GPU_ESTATE, "%s: cube mode is not set "
                "(set_scattered_cube)", what);
  /* the image's own refusals: no camera, a capped or dropped packet, the view */
  CMI_TRY(cmi_gpu_download_image_view(e, view, nullptr, nullptr, nullptr));
  if (e->dust_cube_stale)
    return fail(CMI_GPU_ESTATE, "%s: %s after cube mode was set", what,
                e->dust_cube_stale);
  const DustCubeDev &c = e->dust_cube;
  const size_t nvalue = (size_t)c.npixel * c.nchan;
  RenderArena arena;
  double *ordered = nullptr;
  CMI_TRY(arena.alloc(ordered, nvalue));
  double *dst[3] = {I, Q, U};
  for (int k = 0; k < 3; ++k)
    if (dst[k])
      CMI_TRY(scatter_download_plane(
          e, c.cube + (3 * (size_t)view + k) * nvalue, c.npixel, c.nchan,
          ordered, dst[k]));
  return CMI_GPU_OK;
}

/* ------------------------------------------------------- Lyman alpha -- */

static void lya_free(cmi_gpu_engine *e) {
  (void)hipFree(const_cast<LyaRecord *>(e->lya.records));
  (void)hipFree(e->lya.image);
  (void)hipFree(e->lya.cube);
  (void)hipFree(e->lya_field);
  e->lya_field = nullptr;
  e->lya = LyaDev{};
  e->lya_nviews = 0;
  e->lya_stale = nullptr;
}

int cmi_gpu_reset_lya(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "reset_lya: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (e->lya.nchan) {
    const size_t npix = (size_t)e->lya_nviews * (size_t)e->lya.npixel;
    HIP_TRY(hipMemsetAsync(e->lya.image, 0, npix * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(e->lya.cube, 0,
                           npix * e->lya.nchan * sizeof(double), e->stream));
  }
  if (e->lya_counters)
    HIP_TRY(hipMemsetAsync(e->lya_counters, 0, sizeof(LyaCountersDev),
                           e->stream));
  if (e->lya_field)
    HIP_TRY(hipMemsetAsync(e->lya_field, 0,
                           sizeof(double) * CMI_LYA_FIELD_ROW *
                               (size_t)e->ncell,
                           e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

/* the new mode's device memory in `kept`: the cells' records (from the
 * caller's n_HI and temperature where given), the images, the cubes; the
 * engine's packet queue and counters where they are not there yet */
static int lya_build(cmi_gpu_engine *e, const char *what, RenderArena &kept,
                     RenderArena &scratch, const CellsDev *cells,
                     double sigma_turb, const double *n_HI,
                     const double *temperature, size_t nimage, size_t ncube,
                     LyaRecord *&records, double *&image, double *&cube) {
  const size_t ncell = (size_t)e->ncell;
  double *dn = nullptr, *dT = nullptr;
  unsigned int *ninvalid = nullptr;
  unsigned int bad = 0;
  CMI_TRY(kept.alloc(records, ncell));
  CMI_TRY(kept.alloc(image, nimage));
  CMI_TRY(kept.alloc(cube, ncube));
  CMI_TRY(scratch.alloc(ninvalid, 1));
  if (n_HI)
    CMI_TRY(scratch.upload(dn, n_HI, ncell));
  if (temperature)
    CMI_TRY(scratch.upload(dT, temperature, ncell));
  if (!e->lya_next)
    HIP_TRY(hipMalloc(&e->lya_next, sizeof(unsigned long long)));
  if (!e->lya_counters)
    HIP_TRY(hipMalloc(&e->lya_counters, sizeof(LyaCountersDev)));
  HIP_TRY(hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream));
  LyaRecordArgs a;
  a.number_density = cells->number_density;
  a.x_H = cells->x[0];
  a.n_HI = dn;
  a.temperature = dT ? dT : cells->temperature;
  a.velocity = e->cell_velocities;
  a.sigma_turb = sigma_turb;
  a.sigma_d = e->have_dust_scattering ? e->dust_kappa : 0.;
  a.ncell = e->ncell;
  a.out = records;
  a.ninvalid = ninvalid;
  lya_record_kernel<<<grid_blocks(e, e->ncell, 8), 256, 0, e->stream>>>(a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (bad)
    return fail(CMI_GPU_EINVAL, "%s: %u cell(s) have a Doppler width that is "
                "not positive and finite (T and sigma_turb both 0?) or a "
                "density that is negative or not finite", what, bad);
  return CMI_GPU_OK;
}

int cmi_gpu_set_lyman_alpha(cmi_gpu_engine *e, int32_t nchan, double vmin,
                            double vmax, double sigma_turb, double x_crit,
                            uint64_t max_scatter, const double *n_HI,
                            const double *temperature) {
  static const char *what = "set_lyman_alpha";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  HIP_TRY(hipSetDevice(e->device));
  if (nchan == 0) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    lya_free(e);
    return CMI_GPU_OK;
  }
  CMI_TRY(dust_check_grid(e));
  CMI_TRY(check_have_cells(e, what));
  CMI_TRY(check_camera_set(e, what));
  if (dust_point_camera(e))
    return fail(CMI_GPU_ESTATE, "%s: the point (sky) cameras are not "
                "supported; set_ccd_image or set_ccd_images", what);
  CMI_TRY(check_cell_source_selected(
      e, what, "set_cell_source_field or set_cell_source_line"));
  CMI_TRY(check_cell_source_current(e, what));
  if (e->have_dust_scattering && !e->dust_per_hydrogen)
    return fail(CMI_GPU_ESTATE, "%s: the dust must be given per hydrogen "
                "nucleus (set_dust_scattering_per_hydrogen)", what);
  CMI_TRY(check_sigma_turb(what, sigma_turb));
  if (!(x_crit >= 0.) || !std::isfinite(x_crit))
    return fail(CMI_GPU_EINVAL, "%s: the core-skipping frequency must be >= 0 "
                "and finite", what);
  if (max_scatter < 1 || max_scatter > CMI_LYA_MAX_SCATTER)
    return fail(CMI_GPU_EINVAL, "%s: the cap on scatterings must be 1 to %u "
                "(the packet stream's block counter has 32 bits)", what,
                CMI_LYA_MAX_SCATTER);
  const int32_t nviews = e->dust_nviews;
  LineCubeAxis axis;
  CMI_TRY(line_cube_axis(what, nviews, e->dust.res[0], e->dust.res[1], nchan,
                         vmin, vmax, axis));
  const size_t npixel = dust_image_pixels(e);
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  /* everything new is built aside: a call that fails leaves the previous
   * state in place */
  RenderArena kept, scratch;
  LyaRecord *records = nullptr;
  double *image = nullptr, *cube = nullptr;
  const int rc = lya_build(e, what, kept, scratch, cells, sigma_turb, n_HI,
                           temperature, (size_t)nviews * npixel,
                           (size_t)nviews * npixel * nchan, records, image,
                           cube);
  if (rc)
    return scatter_build_failed(what, rc,
                                kept.out_of_memory || scratch.out_of_memory,
                                nviews, nchan, npixel);
  lya_free(e);
  kept.release();
  LyaDev &l = e->lya;
  l.records = records;
  l.x_crit = x_crit;
  l.x_crit2 = x_crit * x_crit;
  l.max_scatter = (uint32_t)max_scatter;
  l.nchan = nchan;
  l.vmin = axis.vmin;
  l.dv = axis.dv;
  l.npixel = (int64_t)npixel;
  l.image = image;
  l.cube = cube;
  e->lya_nviews = nviews;
  /* the phase function of the dust the records were built with; without dust
   * no event is a dust event, and the constants are those of g = 0.5 */
  e->lya_dust = e->dust;
  if (!e->have_dust_scattering) {
    DustDev &d = e->lya_dust;
    d.hgg = 0.5;
    d.g2 = 0.25;
    d.omg2 = 0.75;
    d.thgg = 1.;
    d.omhgg = 0.5;
    d.od2hgg = 1.;
    d.opg2 = 1.25;
    d.pl = 0.;
    d.sc = 1.;
    d.pc = 0.;
    d.albedo = 0.;
  }
  return cmi_gpu_reset_lya(e);
}

/* what a Lyman-alpha launch or probe asks of the engine; the dust kernels'
 * arguments with the camera as it is now (the mode is stale once it changed) */
static int lya_prepare(cmi_gpu_engine *e, const char *what, DustDev &dust) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  CMI_TRY(check_lya_mode(e, what));
  if (e->lya_stale)
    return fail(CMI_GPU_ESTATE, "%s: %s after Lyman-alpha mode was set; "
                "set_lyman_alpha again", what, e->lya_stale);
  CMI_TRY(check_cell_source_current(e, what));
  HIP_TRY(hipSetDevice(e->device));
  dust = e->lya_dust;
  return CMI_GPU_OK;
}

int cmi_gpu_lya_shoot(cmi_gpu_engine *e, uint32_t seed, uint64_t first_packet,
                      uint64_t n) {
  DustDev dust;
  CMI_TRY(lya_prepare(e, "lya_shoot", dust));
  const ScatterChunks bounds = {CMI_LYA_FIRST_LAUNCH, CMI_LYA_MIN_LAUNCH,
                                CMI_LYA_MAX_LAUNCH, CMI_LYA_STEPS_PER_LAUNCH};
  /* the field's launches are instantiations of their own: without it the
   * kernels are the ones they were */
  const LyaFieldDev field = {e->lya_field, 1. - dust.albedo * dust.hgg};
  return scatter_chunk_loop(
      e, bounds, &e->lya_counters->nsteps, n,
      [&](uint64_t done, uint64_t chunk) {
        HIP_TRY(hipMemsetAsync(e->lya_next, 0, sizeof(unsigned long long),
                               e->stream));
#ifndef CMI_LYA_EVENT_LOOP
        const unsigned blocks = (unsigned)((chunk + 255) / 256);
#else
        const unsigned blocks = (unsigned)std::min<uint64_t>(
            (chunk + 255) / 256, (uint64_t)e->num_cu * CMI_LYA_BLOCKS_PER_CU);
#endif
        return scatter_timed_launch(e, chunk, [&] {
          auto launch = [&](const auto &cam) {
            if (e->lya_field)
              lya_launch_shoot(e, dust, blocks, seed, first_packet + done,
                               chunk, cam, field);
            else
              lya_launch_shoot(e, dust, blocks, seed, first_packet + done,
                               chunk, cam);
          };
          if (e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS)
            launch(scatter_camera<DUST_CAMERA_PARALLEL_VIEWS>(e,
                                                              e->sky_camera));
          else
            launch(DustCamera<DUST_CAMERA_PARALLEL>());
        });
      });
}

int cmi_gpu_get_lya_counters(cmi_gpu_engine *e, uint64_t *counters) {
  if (!e || !counters)
    return fail(CMI_GPU_EINVAL, "get_lya_counters: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  LyaCountersDev c = {};
  if (e->lya_counters)
    HIP_TRY(hipMemcpy(&c, e->lya_counters, sizeof c, hipMemcpyDeviceToHost));
  counters[0] = c.nsteps;
  counters[1] = c.nhydrogen;
  counters[2] = c.ndust;
  counters[3] = c.nrejections;
  counters[4] = c.natomics;
  counters[5] = c.ncapped;
  counters[6] = c.npackets;
  return CMI_GPU_OK;
}

int cmi_gpu_download_lya_view(cmi_gpu_engine *e, int32_t view, double *image,
                              double *cube) {
  static const char *what = "download_lya_view";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  CMI_TRY(check_lya_mode(e, what));
  if (e->lya_stale)
    return fail(CMI_GPU_ESTATE, "%s: %s after Lyman-alpha mode was set", what,
                e->lya_stale);
  CMI_TRY(check_view(what, view, e->lya_nviews));
  uint64_t c[7];
  CMI_TRY(cmi_gpu_get_lya_counters(e, c));
  if (c[5])
    return fail(CMI_GPU_ESTATE, "%s: %llu packet(s) reached the cap of %u "
                "scatterings; the image is incomplete", what,
                (unsigned long long)c[5], e->lya.max_scatter);
  const LyaDev &l = e->lya;
  const size_t npixel = (size_t)l.npixel;
  const size_t nvalue = npixel * l.nchan;
  if (image)
    HIP_TRY(hipMemcpy(image, l.image + (size_t)view * npixel,
                      npixel * sizeof(double), hipMemcpyDeviceToHost));
  if (!cube)
    return CMI_GPU_OK;
  RenderArena arena;
  double *ordered = nullptr;
  CMI_TRY(arena.alloc(ordered, nvalue));
  return scatter_download_plane(e, l.cube + (size_t)view * nvalue, l.npixel,
                                l.nchan, ordered, cube);
}

int cmi_gpu_lya_probe(cmi_gpu_engine *e, int32_t kind, uint32_t seed,
                      uint64_t first_packet, int64_t n, const double *in,
                      double *out, int32_t max_events) {
  static const char *what = "lya_probe";
  if (!e || n < 0 || !out || kind < 0 || kind > LYA_PROBE_TRACE ||
      max_events < 0 || n > (1 << 24))
    return fail(CMI_GPU_EINVAL, "%s: bad argument", what);
  static const int in_width[4] = {4, 7, 2, 0};
  const int width =
      kind == LYA_PROBE_TRACE
          ? CMI_LYA_TRACE_HEADER + CMI_LYA_TRACE_ROW * max_events
          : 2;
  if (in_width[kind] && !in)
    return fail(CMI_GPU_EINVAL, "%s: input rows missing", what);
  DustDev dust;
  CMI_TRY(lya_prepare(e, what, dust));
  /* with several views a trace follows the selected one through the single
   * camera's kernel (it writes to no image) */
  if (e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS)
    dust_put_view(dust, e->dust_views[e->dust_probe_view]);
  if (n == 0)
    return CMI_GPU_OK;
  return scatter_probe_rows(
      e, n, in_width[kind], width, in, out,
      [&](const double *rows_in, double *rows_out, int64_t first, int64_t m) {
        lya_probe_kernel<DUST_CAMERA_PARALLEL>
            <<<(unsigned)((m + 63) / 64), 64, 0, e->stream>>>(
                e->grid, dust, e->cell_source,
                DustCamera<DUST_CAMERA_PARALLEL>(), e->lya, kind, seed,
                first_packet + first, m, width, rows_in, rows_out, max_events);
      });
}

int cmi_gpu_set_lya_field(cmi_gpu_engine *e, int32_t enable) {
  static const char *what = "set_lya_field";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  CMI_TRY(check_lya_mode(e, what));
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t bytes = sizeof(double) * CMI_LYA_FIELD_ROW * (size_t)e->ncell;
  if (!enable) {
    (void)hipFree(e->lya_field);
    e->lya_field = nullptr;
    return CMI_GPU_OK;
  }
  if (!e->lya_field) {
    /* hipMalloc's 256-byte alignment makes every row one 64-byte line */
    double *rows = nullptr;
    const hipError_t err = hipMalloc(&rows, bytes);
    if (err == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      return fail(CMI_GPU_ENOMEM, "%s: %zu bytes of rows do not fit into the "
                  "device's memory", what, bytes);
    }
    HIP_TRY(err);
    e->lya_field = rows;
  }
  HIP_TRY(hipMemsetAsync(e->lya_field, 0, bytes, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

/* what a reader of the field asks: the mode on and not stale, the field on,
 * no capped packet */
static int lya_field_ready(cmi_gpu_engine *e, const char *what) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  CMI_TRY(check_lya_mode(e, what));
  if (!e->lya_field)
    return fail(CMI_GPU_ESTATE, "%s: the radiation field is off "
                "(set_lya_field)", what);
  if (e->lya_stale)
    return fail(CMI_GPU_ESTATE, "%s: %s after Lyman-alpha mode was set", what,
                e->lya_stale);
  uint64_t c[7];
  CMI_TRY(cmi_gpu_get_lya_counters(e, c));
  if (c[5])
    return fail(CMI_GPU_ESTATE, "%s: %llu packet(s) reached the cap of %u "
                "scatterings; the field is incomplete", what,
                (unsigned long long)c[5], e->lya.max_scatter);
  return CMI_GPU_OK;
}

int cmi_gpu_download_lya_field(cmi_gpu_engine *e, double *rows) {
  static const char *what = "download_lya_field";
  if (e && !rows)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(lya_field_ready(e, what));
  HIP_TRY(hipMemcpy(rows, e->lya_field,
                    sizeof(double) * CMI_LYA_FIELD_ROW * (size_t)e->ncell,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

int cmi_gpu_lya_spin_temperature(cmi_gpu_engine *e,
                                 double luminosity_per_packet,
                                 double background_temperature,
                                 int32_t collisions, double *P_alpha,
                                 double *T_s) {
  static const char *what = "lya_spin_temperature";
  if (!e || !T_s)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  if (!(luminosity_per_packet > 0.) || !std::isfinite(luminosity_per_packet))
    return fail(CMI_GPU_EINVAL, "%s: the luminosity per packet must be "
                "positive and finite (%.17g)", what, luminosity_per_packet);
  if (!(background_temperature > 0.) || !std::isfinite(background_temperature))
    return fail(CMI_GPU_EINVAL, "%s: the background temperature must be "
                "positive and finite (%.17g)", what, background_temperature);
  CMI_TRY(lya_field_ready(e, what));
  if (e->lya.x_crit > 0.)
    return fail(CMI_GPU_ESTATE, "%s: the mode was set with core skipping "
                "(x_crit = %g): the skipped scatterings are missing from the "
                "scattering rate", what, e->lya.x_crit);
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  const size_t ncell = (size_t)e->ncell;
  RenderArena arena;
  double *out = nullptr;
  CMI_TRY(arena.alloc(out, 2 * ncell));
  LyaCouplingArgs a;
  a.rows = e->lya_field;
  a.records = e->lya.records;
  a.number_density = cells->number_density;
  a.temperature = cells->temperature;
  a.x_H0 = cells->x[0];
  a.x_He0 = cells->x[1];
  a.A_He = e->model.abundance[0];
  a.scale = luminosity_per_packet;
  a.background = background_temperature;
  a.cell_volume =
      e->grid.cellside[0] * e->grid.cellside[1] * e->grid.cellside[2];
  a.collisions = collisions ? 1 : 0;
  a.ncell = e->ncell;
  a.P_alpha = out;
  a.T_s = out + ncell;
  lya_coupling_kernel<<<(unsigned)((ncell + 255) / 256), 256, 0, e->stream>>>(
      a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (P_alpha)
    HIP_TRY(hipMemcpy(P_alpha, out, sizeof(double) * ncell,
                      hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(T_s, out + ncell, sizeof(double) * ncell,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

int cmi_gpu_lyman_alpha_emissivity(cmi_gpu_engine *e, double *out) {
  static const char *what = "lyman_alpha_emissivity";
  if (!e || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  CMI_TRY(check_have_cells(e, what));
  HIP_TRY(hipSetDevice(e->device));
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  RenderArena arena;
  double *dev = nullptr;
  CMI_TRY(arena.alloc(dev, (size_t)e->ncell));
  lya_emissivity_kernel<<<(unsigned)((e->ncell + 255) / 256), 256, 0,
                          e->stream>>>(
      cells->number_density, cells->temperature, cells->x[0], cells->x[1],
      e->model.abundance[0], e->ncell, dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, dev, sizeof(double) * (size_t)e->ncell,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

#endif
