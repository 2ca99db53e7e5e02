/*
 * EmissionProducts.hpp - what the emission mode renders for a block of
 * EmissionSettings.hpp, written once for both blocks (render_products): the
 * lines' images or maps with their cubes, the radio continuum, the H I cube
 * and the scattered light. What differs between the blocks is the camera:
 * the parallel views of EmissionImages: (ParallelViews, which alone serve the
 * Lyman-alpha run) and the observers of EmissionSkyMaps: (SkyObservers).
 * A new product is one step in render_products and one call per camera.
 */
#ifndef CMI_EMISSIONPRODUCTS_HPP
#define CMI_EMISSIONPRODUCTS_HPP

#include "EmissionSettings.hpp"

namespace cmi {
namespace emission {

/* what the steps of a run share: the engine, destroyed on every way out, the
 * progress lines of --verbose and the names of the files written */
struct Run {
  cmi_gpu_engine *engine = nullptr;
  const bool write_output, verbose;
  std::string written;

  Run(bool write_output, bool verbose)
      : write_output(write_output), verbose(verbose) {}
  Run(const Run &) = delete;
  ~Run() {
    if (engine)
      cmi_gpu_destroy(engine);
  }

  /* the first error of the engine ends the run, with its message */
  void check(int rc) const {
    if (rc != CMI_GPU_OK)
      throw std::runtime_error(std::string("emissivity calculation: ") +
                               cmi_gpu_last_error());
  }
  void status(const std::string &text) const {
    if (verbose)
      std::cout << text << std::endl;
  }
  void wrote(const std::string &filename) { written += " " + filename; }
};

/* what the cameras have in common: the block, the pixels of a view, the
 * words of the block's messages. A camera adds nviews() and, for view v, the
 * renderers of the engine, install() for the Monte Carlo runs and
 * scale_scattered() for what they leave. */
struct Camera {
  const ProductSettings &s;
  const long long nx, ny;
  const char *noun, *plural, *hi_cubes, *shooting;

  size_t npixel() const { return (size_t)nx * (size_t)ny; }
  /* a call's output holds at most 2^28 values */
  void check_size(double nplane, const std::string &what) const {
    if (nplane * (double)npixel() > (double)(1ll << 28))
      throw ParameterError(s.block + ": " + what + " of " +
                           std::to_string(nx) + " x " + std::to_string(ny) +
                           " pixels: more than 2^28 values in one call");
  }
};

/* EmissionImages: parallel projections along (theta, phi) */
struct ParallelViews : Camera {
  const ImageSettings &img;
  std::vector<double> theta, phi, anchors, sides;
  /* velocities ahead of the cubes: a field at rest is not uploaded */
  static const bool uploads_rest = false;

  /* per view, default image: the rectangle around the box's projected
   * corners */
  ParallelViews(const ImageSettings &img,
                const std::array<double, 3> &box_anchor,
                const std::array<double, 3> &box_sides)
      : Camera{img, img.nx, img.ny, "image", "images", "cubes",
               "through the dust"},
        img(img) {
    for (const ImageSettings::View &view : img.views) {
      theta.push_back(view.theta);
      phi.push_back(view.phi);
      const double st = std::sin(view.theta), ct = std::cos(view.theta),
                   sp = std::sin(view.phi), cp = std::cos(view.phi);
      const double ex[3] = {-sp, cp, 0.};
      const double ey[3] = {-ct * cp, -ct * sp, st};
      double lo[2] = {HUGE_VAL, HUGE_VAL}, hi[2] = {-HUGE_VAL, -HUGE_VAL};
      for (int corner = 0; corner < 8; ++corner) {
        double p[2] = {0., 0.};
        for (int a = 0; a < 3; ++a) {
          const double x = box_anchor[a] + ((corner >> a) & 1) * box_sides[a];
          p[0] += x * ex[a];
          p[1] += x * ey[a];
        }
        for (int k = 0; k < 2; ++k) {
          lo[k] = std::min(lo[k], p[k]);
          hi[k] = std::max(hi[k], p[k]);
        }
      }
      double anchor[2];
      for (int k = 0; k < 2; ++k)
        anchor[k] = view.have_anchor[k] ? view.anchor[k] : lo[k];
      anchors.insert(anchors.end(), anchor, anchor + 2);
      for (int k = 0; k < 2; ++k)
        sides.push_back(view.have_sides[k] ? view.sides[k]
                                           : hi[k] - anchor[k]);
    }
  }

  size_t nviews() const { return theta.size(); }
  void render_lines(const Run &run, const std::vector<int32_t> &lines,
                    size_t v, double *images) const {
    run.check(cmi_gpu_render_line_images(
        run.engine, (int32_t)lines.size(), lines.data(), theta[v], phi[v],
        (int32_t)nx, (int32_t)ny, &anchors[2 * v], &sides[2 * v],
        (int32_t)img.supersample, img.dust_cross_section, images));
  }
  void render_line_cubes(const Run &run, const std::vector<int32_t> &lines,
                         size_t v, double *cubes) const {
    run.check(cmi_gpu_render_line_cube(
        run.engine, (int32_t)lines.size(), lines.data(), theta[v], phi[v],
        (int32_t)nx, (int32_t)ny, &anchors[2 * v], &sides[2 * v],
        (int32_t)img.supersample, img.dust_cross_section, (int32_t)img.nchan,
        img.vmin, img.vmax, img.sigma_turb, cubes));
  }
  void render_continuum(const Run &run, size_t v, double *images) const {
    run.check(cmi_gpu_render_continuum_images(
        run.engine, (int32_t)img.continuum_frequencies.size(),
        img.continuum_frequencies.data(), img.continuum_background.data(),
        theta[v], phi[v], (int32_t)nx, (int32_t)ny, &anchors[2 * v],
        &sides[2 * v], (int32_t)img.supersample, images));
  }
  void render_hi_cube(const Run &run, size_t v, int32_t spin_mode,
                      const double *spin, double *cube) const {
    run.check(cmi_gpu_render_hi_cube(
        run.engine, theta[v], phi[v], (int32_t)nx, (int32_t)ny,
        &anchors[2 * v], &sides[2 * v], (int32_t)img.supersample,
        (int32_t)img.nchan, img.vmin, img.vmax, img.sigma_turb, spin_mode,
        spin, img.hi_free_free ? 1 : 0, img.hi_background_temperature, cube));
  }
  /* one view: the single camera, as ever; several: one run fills them all */
  void install(const Run &run) const {
    run.check(nviews() == 1
                  ? cmi_gpu_set_ccd_image(run.engine, theta[0], phi[0],
                                          (int32_t)nx, (int32_t)ny,
                                          anchors.data(), sides.data())
                  : cmi_gpu_set_ccd_images(
                        run.engine, (int32_t)nviews(), theta.data(),
                        phi.data(), (int32_t)nx, (int32_t)ny, anchors.data(),
                        sides.data()));
  }
  /* (the scattered cubes: observers at rest) */
  const double *observer_velocities() const { return nullptr; }
  /* brings n downloaded values of view v, pixel i % npixel(), from a run of
   * luminosity `total` to W m^-2 sr^-1: x L_total / (packets x pixel area).
   * With `leave_factor` the values stay and the factor is returned for
   * write_image to multiply in (it does not for a PGM). */
  double scale_scattered(size_t v, double total, double *values, size_t n,
                         bool leave_factor) const {
    const double pixel_area =
        sides[2 * v] * sides[2 * v + 1] / ((double)nx * (double)ny);
    const double scale = total / ((double)img.npackets * pixel_area);
    if (leave_factor)
      return scale;
    for (size_t i = 0; i < n; ++i)
      values[i] *= scale;
    return 1.;
  }
};

/* EmissionSkyMaps: equirectangular maps around observers */
struct SkyObservers : Camera {
  const SkyMapSettings &sky;
  const std::vector<double> &origins, &frames, &velocities, &radii;
  /* the pixels' solid angles, [view][pixel], once install() has run */
  std::vector<double> omega;
  /* velocities ahead of the cubes: a field at rest is uploaded as null,
   * which clears what EmissionImages: left */
  static const bool uploads_rest = true;

  explicit SkyObservers(const SkyMapSettings &sky)
      : Camera{sky, sky.nlon, sky.nlat, "map", "sky maps", "sky cubes",
               "towards the observer"},
        sky(sky), origins(sky.positions), frames(sky.frames),
        velocities(sky.velocities), radii(sky.exclusion_radii) {}

  size_t nviews() const { return radii.size(); }
  void render_lines(const Run &run, const std::vector<int32_t> &lines,
                    size_t v, double *maps) const {
    run.check(cmi_gpu_render_line_sky_map(
        run.engine, (int32_t)lines.size(), lines.data(), &origins[3 * v],
        &frames[9 * v], sky.lon[0], sky.lon[1], sky.lat[0], sky.lat[1],
        (int32_t)nx, (int32_t)ny, sky.dust_cross_section, maps));
  }
  void render_line_cubes(const Run &run, const std::vector<int32_t> &lines,
                         size_t v, double *cubes) const {
    run.check(cmi_gpu_render_line_sky_map_cube(
        run.engine, (int32_t)lines.size(), lines.data(), &origins[3 * v],
        &frames[9 * v], sky.lon[0], sky.lon[1], sky.lat[0], sky.lat[1],
        (int32_t)nx, (int32_t)ny, sky.dust_cross_section, &velocities[3 * v],
        (int32_t)sky.nchan, sky.vmin, sky.vmax, sky.sigma_turb, cubes));
  }
  void render_continuum(const Run &run, size_t v, double *maps) const {
    run.check(cmi_gpu_render_continuum_sky_map(
        run.engine, (int32_t)sky.continuum_frequencies.size(),
        sky.continuum_frequencies.data(), sky.continuum_background.data(),
        &origins[3 * v], (int32_t)nx, (int32_t)ny, sky.lon.data(),
        sky.lat.data(), &frames[9 * v], maps));
  }
  /* (the spin temperature is always the block's own: the coupled one belongs
   * to the Lyman-alpha run of EmissionImages) */
  void render_hi_cube(const Run &run, size_t v, int32_t spin_mode,
                      const double *spin, double *cube) const {
    run.check(cmi_gpu_render_hi_sky_map_cube(
        run.engine, &origins[3 * v], &frames[9 * v], sky.lon[0], sky.lon[1],
        sky.lat[0], sky.lat[1], (int32_t)nx, (int32_t)ny, &velocities[3 * v],
        (int32_t)sky.nchan, sky.vmin, sky.vmax, sky.sigma_turb, spin_mode,
        spin, sky.hi_free_free ? 1 : 0, sky.hi_background_temperature, cube));
  }
  /* one observer: the single camera, as ever; several: one run fills them
   * all */
  void install(const Run &run) {
    omega.resize(nviews() * npixel());
    for (size_t v = 0; v < nviews(); ++v)
      run.check(cmi_gpu_sky_map_directions(
          &frames[9 * v], sky.lon[0], sky.camera_lon_max, sky.lat[0],
          sky.lat[1], (int32_t)nx, (int32_t)ny, nullptr,
          &omega[v * npixel()]));
    run.check(nviews() == 1
                  ? cmi_gpu_set_sky_camera(
                        run.engine, origins.data(), frames.data(), sky.lon[0],
                        sky.camera_lon_max, sky.lat[0], sky.lat[1],
                        (int32_t)nx, (int32_t)ny, radii[0],
                        sky.direct_light ? 1 : 0)
                  : cmi_gpu_set_sky_cameras(
                        run.engine, (int32_t)nviews(), origins.data(),
                        frames.data(), sky.lon[0], sky.camera_lon_max,
                        sky.lat[0], sky.lat[1], (int32_t)nx, (int32_t)ny,
                        radii.data(), sky.direct_light ? 1 : 0));
  }
  const double *observer_velocities() const { return velocities.data(); }
  /* as ParallelViews': x L_total / packets / the pixel's solid angle, in the
   * order the Python call multiplies. No factor is the same for all pixels,
   * so none is left: a PGM shows the scaled values. */
  double scale_scattered(size_t v, double total, double *values, size_t n,
                         bool) const {
    const double per_packet = total / (double)sky.npackets;
    const double *pixel_omega = &omega[v * npixel()];
    for (size_t i = 0; i < n; ++i)
      values[i] = values[i] * per_packet / pixel_omega[i % npixel()];
    return 1.;
  }
};

/* the flagged lines as images or maps of every view and, with "velocity
 * channels", those that are the line of one ion as cubes; `velocities` is
 * the block's field in the engine's cell order, empty for one at rest */
template <class Cam>
void render_lines(Run &run, const Cam &cam,
                  const std::vector<int32_t> &lines,
                  const std::vector<double> &velocities) {
  const ProductSettings &s = cam.s;
  const size_t npixel = cam.npixel();
  std::vector<double> images(lines.size() * npixel);
  std::vector<int32_t> cube_lines;
  std::vector<double> cube;
  if (s.cubes) {
    for (const int32_t line : lines)
      if (cmi_gpu_emission_line_atomic_weight(line) > 0.)
        cube_lines.push_back(line);
      else
        std::cerr << s.block << ": " << Settings::line_name(line)
                  << " is not the line of one ion: no cube, the " << cam.noun
                  << " alone" << std::endl;
    cam.check_size((double)cube_lines.size() * (double)s.nchan,
                   std::to_string(cube_lines.size()) + " cubes of " +
                       std::to_string(s.nchan) + " channels");
    cube.resize(cube_lines.size() * (size_t)s.nchan * npixel);
    if ((!cube_lines.empty() || s.hi_cube) &&
        (cam.uploads_rest || !velocities.empty()))
      run.check(cmi_gpu_set_cell_velocities(
          run.engine, velocities.empty() ? nullptr : velocities.data()));
  }
  for (size_t v = 0; v < cam.nviews(); ++v) {
    cam.render_lines(run, lines, v, images.data());
    for (size_t k = 0; run.write_output && k < lines.size(); ++k)
      run.wrote(write_image(s.file_name(Settings::line_name(lines[k]), "", v),
                            s.type, &images[k * npixel], cam.nx, cam.ny, 1.));
    if (cube_lines.empty())
      continue;
    cam.render_line_cubes(run, cube_lines, v, cube.data());
    for (size_t k = 0; run.write_output && k < cube_lines.size(); ++k)
      run.wrote(write_cube(
          s.file_name(Settings::line_name(cube_lines[k]), "_cube", v),
          &cube[k * (size_t)s.nchan * npixel], s.nchan, cam.nx, cam.ny));
  }
}

/* "continuum frequencies": the free-free emission at every frequency */
template <class Cam> void render_continuum(Run &run, const Cam &cam) {
  const ProductSettings &s = cam.s;
  if (!s.continuum)
    return;
  run.status(std::string("Rendering radio continuum ") + cam.plural + "...");
  const size_t nf = s.continuum_frequencies.size();
  cam.check_size((double)nf, std::to_string(nf) + " continuum frequencies");
  std::vector<double> continuum(nf * cam.npixel());
  for (size_t v = 0; v < cam.nviews(); ++v) {
    cam.render_continuum(run, v, continuum.data());
    if (run.write_output)
      run.wrote(write_cube(s.file_name("continuum", "", v), continuum.data(),
                           (long long)nf, cam.nx, cam.ny));
  }
  if (run.write_output)
    run.wrote(s.write_continuum_frequencies(
        s.file_name("continuum", "_frequencies")));
}

/* "HI cube": the 21-cm line, with the spin temperature of the block's keys
 * or, if `coupled_spin` is not null, with that of every cell */
template <class Cam>
void render_hi_cubes(Run &run, const Cam &cam, const double *coupled_spin) {
  const ProductSettings &s = cam.s;
  if (!s.hi_cube)
    return;
  run.status(std::string("Rendering H I ") + cam.hi_cubes + "...");
  cam.check_size((double)s.nchan, "an H I cube of " + std::to_string(s.nchan) +
                                      " channels");
  std::vector<double> hi((size_t)s.nchan * cam.npixel());
  for (size_t v = 0; v < cam.nviews(); ++v) {
    cam.render_hi_cube(run, v, coupled_spin ? 2 : s.hi_spin_mode,
                       coupled_spin ? coupled_spin : &s.hi_spin_temperature,
                       hi.data());
    if (run.write_output)
      run.wrote(write_cube(s.file_name("HI", "_cube", v), hi.data(), s.nchan,
                           cam.nx, cam.ny));
  }
}

/* "scattering": one Monte Carlo run per flagged line fills I, Q and U of all
 * views and, with "scattered cubes", the cubes of the lines of one ion */
template <class Cam>
void shoot_scattered_light(Run &run, Cam &cam,
                           const std::vector<int32_t> &lines) {
  static const char *stokes[3] = {"_I", "_Q", "_U"};
  const ProductSettings &s = cam.s;
  if (!s.scattering)
    return;
  run.status(std::string("Shooting the lines' packets ") + cam.shooting +
             "...");
  run.check(cmi_gpu_set_dust_scattering_per_hydrogen(
      run.engine, s.asymmetry, s.polarisation, s.albedo,
      s.dust_cross_section));
  cam.install(run);
  const size_t npixel = cam.npixel(), nvalue = (size_t)s.nchan * npixel;
  std::vector<double> iqu(3 * npixel);
  std::vector<double> cube(s.scattered_cubes ? 3 * nvalue : 0);
  for (const int32_t line : lines) {
    const std::string name = Settings::line_name(line);
    run.check(cmi_gpu_set_cell_source_line(run.engine, line));
    /* cube mode for the lines of one ion (it resets the image); the cells'
     * velocities are those the ray-traced cubes were given */
    const bool with_cube =
        s.scattered_cubes && cmi_gpu_emission_line_atomic_weight(line) > 0.;
    if (s.scattered_cubes)
      run.check(cmi_gpu_set_scattered_cube(
          run.engine, with_cube ? (int32_t)s.nchan : 0, s.vmin, s.vmax,
          s.sigma_turb, nullptr, cam.observer_velocities()));
    run.check(cmi_gpu_reset_image(run.engine));
    run.check(cmi_gpu_dust_shoot(run.engine, (uint32_t)s.seed, 0,
                                 (uint64_t)s.npackets));
    double total = 0.;
    run.check(cmi_gpu_get_cell_source(run.engine, &total, nullptr, nullptr));
    for (size_t v = 0; v < cam.nviews(); ++v) {
      run.check(cmi_gpu_download_image_view(run.engine, (int32_t)v, &iqu[0],
                                            &iqu[npixel], &iqu[2 * npixel]));
      const double factor =
          cam.scale_scattered(v, total, iqu.data(), iqu.size(), true);
      for (int j = 0; run.write_output && j < 3; ++j)
        run.wrote(write_image(
            s.file_name(name, "", v, std::string("_scattered") + stokes[j]),
            s.type, &iqu[j * npixel], cam.nx, cam.ny, factor));
      if (!with_cube)
        continue;
      run.check(cmi_gpu_download_cube_view(run.engine, (int32_t)v, &cube[0],
                                           &cube[nvalue], &cube[2 * nvalue]));
      cam.scale_scattered(v, total, cube.data(), cube.size(), false);
      for (int j = 0; run.write_output && j < 3; ++j)
        run.wrote(write_cube(
            s.file_name(name, "", v,
                        std::string("_scattered_cube") + stokes[j]),
            &cube[j * nvalue], s.nchan, cam.nx, cam.ny));
    }
  }
  if (s.scattered_cubes)
    run.check(cmi_gpu_set_scattered_cube(run.engine, 0, 0., 1., 0., nullptr,
                                         nullptr));
}

/* "Lyman alpha" of EmissionImages: packets from the
 * cells' recombinations through the cells' own H I and the block's dust, as
 * an image and a cube per view; the field the run leaves in the cells and
 * the spin temperature it gives if the block asks for them */
struct LymanAlpha {
  const ParallelViews &cam;
  const std::array<long long, 3> &ncell;
  const std::array<double, 3> &box_sides;
  const std::vector<double> &velocities; /* the block's, as render_lines' */
  /* with "HI Lyman alpha coupling": the cells' spin temperatures */
  std::vector<double> coupled_spin;

  /* the field: rows {L, S_H, S_d, G[3], N_H, N_d} of the engine -> [5][ncell]
   * in physical units; the rate per atom is the engine's (it knows the
   * records' n_HI), 0 if the core is skipped */
  void download_field(Run &run, double total) {
    const ImageSettings &img = cam.img;
    const size_t size = (size_t)(ncell[0] * ncell[1] * ncell[2]);
    const double per_packet = total / (double)img.npackets;
    const double volume = (box_sides[0] / ncell[0]) *
                          (box_sides[1] / ncell[1]) *
                          (box_sides[2] / ncell[2]);
    const double per_volume = per_packet / (299792458. * volume);
    std::vector<double> rows(8 * size), field(5 * size, 0.), spin(size);
    run.check(cmi_gpu_download_lya_field(run.engine, rows.data()));
    if (!(img.lya_core_skip > 0.))
      run.check(cmi_gpu_lya_spin_temperature(
          run.engine, per_packet,
          img.lya_coupling ? img.hi_background_temperature : 1.,
          img.lya_coupling ? 1 : 0, field.data() + size, spin.data()));
    for (size_t c = 0; c < size; ++c) {
      field[c] = rows[8 * c] * per_volume;
      for (size_t a = 0; a < 3; ++a)
        field[(2 + a) * size + c] = rows[8 * c + 3 + a] * per_volume;
    }
    if (run.write_output) {
      run.wrote(write_cube(img.file_name("LymanAlpha", "_field"), field.data(),
                           5 * ncell[0], ncell[1], ncell[2]));
      if (img.lya_coupling)
        run.wrote(write_cube(img.file_name("HI", "_spin_temperature"),
                             spin.data(), ncell[0], ncell[1], ncell[2]));
    }
    if (img.lya_coupling)
      coupled_spin.swap(spin);
  }

  void shoot(Run &run) {
    const ImageSettings &img = cam.img;
    run.status("Shooting the Lyman alpha packets through the H I...");
    /* the source: the cells' recombinations; the scatterers: the cells' own
     * H I at their temperatures, and the block's dust */
    std::vector<double> source((size_t)(ncell[0] * ncell[1] * ncell[2]));
    run.check(cmi_gpu_lyman_alpha_emissivity(run.engine, source.data()));
    run.check(cmi_gpu_set_dust_scattering_per_hydrogen(
        run.engine, img.asymmetry, img.polarisation, img.albedo,
        img.dust_cross_section));
    cam.install(run);
    if (!velocities.empty())
      run.check(cmi_gpu_set_cell_velocities(run.engine, velocities.data()));
    run.check(cmi_gpu_set_cell_source_field(run.engine, source.data()));
    run.check(cmi_gpu_set_lyman_alpha(
        run.engine, (int32_t)img.nchan, img.vmin, img.vmax, img.sigma_turb,
        img.lya_core_skip, (uint64_t)img.lya_max_scatter, nullptr, nullptr));
    if (img.lya_field)
      run.check(cmi_gpu_set_lya_field(run.engine, 1));
    run.check(cmi_gpu_lya_shoot(run.engine, (uint32_t)img.seed, 0,
                                (uint64_t)img.npackets));
    double total = 0.;
    run.check(cmi_gpu_get_cell_source(run.engine, &total, nullptr, nullptr));
    std::vector<double> image(cam.npixel()),
        cube((size_t)img.nchan * cam.npixel());
    for (size_t v = 0; v < cam.nviews(); ++v) {
      run.check(cmi_gpu_download_lya_view(run.engine, (int32_t)v, image.data(),
                                          cube.data()));
      const double factor =
          cam.scale_scattered(v, total, image.data(), image.size(), true);
      cam.scale_scattered(v, total, cube.data(), cube.size(), false);
      if (!run.write_output)
        continue;
      run.wrote(write_image(img.file_name("LymanAlpha", "_image", v), img.type,
                            image.data(), cam.nx, cam.ny, factor));
      run.wrote(write_cube(img.file_name("LymanAlpha", "_cube", v),
                           cube.data(), img.nchan, cam.nx, cam.ny));
    }
    if (img.lya_field)
      download_field(run, total);
    run.check(cmi_gpu_set_lyman_alpha(run.engine, 0, 0., 1., 0., 0., 1,
                                      nullptr, nullptr));
  }
};

/* everything a block asks for, in the order the files are listed. `lya` is
 * null without "Lyman alpha: true" (and for the sky maps, which refuse it);
 * with "HI Lyman alpha coupling" its run comes ahead of the H I cube, which
 * takes the spin temperature it leaves. */
template <class Cam>
void render_products(Run &run, Cam &cam, const std::vector<int32_t> &lines,
                     const std::vector<double> &velocities,
                     LymanAlpha *lya = nullptr) {
  run.status(std::string("Rendering emission line ") + cam.plural + "...");
  render_lines(run, cam, lines, velocities);
  render_continuum(run, cam);
  const bool coupled = lya && lya->cam.img.lya_coupling;
  if (coupled)
    lya->shoot(run);
  render_hi_cubes(run, cam, coupled ? lya->coupled_spin.data() : nullptr);
  shoot_scattered_light(run, cam, lines);
  if (lya && !coupled)
    lya->shoot(run);
}

} // namespace emission
} // namespace cmi

#endif
