/*
 * EmissionSettings.hpp - the parameter blocks of the emission mode
 * (EmissivityCalculationSimulation.hpp) and what their keys mean.
 *
 * The emission lines flagged in "EmissivityValues:<name>" are computed and
 * added to the snapshot. Beyond the reference: if - and only if - the
 * parameter file has an
 * "EmissionImages:" block, every flagged line is also rendered as a
 * line-of-sight map (cmi_gpu_render_line_images) and written to
 * <output folder>/<filename prefix>_<LineName>.dat or .pgm:
 *   EmissionImages:view theta / view phi         0. degrees / 0. degrees
 *   EmissionImages:image width / image height    200 / 200
 *   EmissionImages:anchor x / anchor y / sides x / sides y
 *                    the bounding rectangle of the box's projected corners
 *   EmissionImages:supersampling                 1
 *   EmissionImages:dust cross section per hydrogen   0. m^2
 *   EmissionImages:type                          BinaryArray (or PGM)
 *   EmissionImages:filename prefix               line_image
 *   EmissionImages:output folder                 .
 * With "EmissionImages:scattering: true" every flagged line is also shot as
 * a Monte Carlo run (cmi_gpu_set_cell_source_line, cmi_gpu_dust_shoot): its
 * packets start in the cells in proportion to the line's emissivity, scatter
 * off dust of the same cross section per hydrogen and are peeled off towards
 * the observer. I, Q and U are written next to the ray-traced image as
 * <prefix>_<LineName>_scattered_I / _Q / _U, scaled by L_total / (packets x
 * pixel area) to W m^-2 sr^-1 like it. Read only then:
 *   EmissionImages:number of packets             1000000
 *   EmissionImages:random seed                   42
 *   EmissionImages:dust albedo / dust asymmetry / dust peak linear
 *                    polarisation: required if the cross section is > 0
 * If the file has an "EmissionSkyMaps:" block, every flagged line is
 * rendered as an equirectangular map of the sky around an observer inside
 * or near the box (cmi_gpu_render_line_sky_map; pixel (i, j) of longitude i
 * and latitude j at i * nlat + j) and written to <output folder>/<filename
 * prefix>_<LineName>.dat or .pgm:
 *   EmissionSkyMaps:observer position            required, a vector of lengths
 *   EmissionSkyMaps:number of longitude pixels / number of latitude pixels
 *                                                360 / 180
 *   EmissionSkyMaps:longitude range              [-180. degrees, 180. degrees]
 *   EmissionSkyMaps:latitude range               [-90. degrees, 90. degrees]
 *   EmissionSkyMaps:frame pole                   [0, 0, 1]
 *   EmissionSkyMaps:frame zero longitude         [1, 0, 0]
 *                    orthonormalised by Gram-Schmidt (the pole is kept, the
 *                    zero of longitude is made perpendicular to it, the
 *                    third axis is pole x zero longitude); refused if parallel
 *   EmissionSkyMaps:dust cross section per hydrogen   0. m^2
 *   EmissionSkyMaps:type / filename prefix / output folder
 *                                                BinaryArray / sky_map / .
 * With "EmissionSkyMaps:scattering: true" every flagged line is also shot as
 * a Monte Carlo run peeled off towards the observer (cmi_gpu_set_sky_camera,
 * cmi_gpu_set_cell_source_line, cmi_gpu_dust_shoot) through dust of the same
 * cross section per hydrogen; I, Q and U are written next to the ray-traced
 * map as <prefix>_<LineName>_scattered_I / _Q / _U, scaled by L_total /
 * (packets x the pixel's solid angle) to W m^-2 sr^-1 like it. The longitude
 * range may then not be wider than 360 degrees. Read only then:
 *   EmissionSkyMaps:number of packets            1000000
 *   EmissionSkyMaps:random seed                  42
 *   EmissionSkyMaps:dust albedo / dust asymmetry / dust peak linear
 *                    polarisation: required if the cross section is > 0
 *   EmissionSkyMaps:exclusion radius             required, a length: events
 *                    nearer to the observer than this add nothing
 *   EmissionSkyMaps:direct light                 true (false: the scattered
 *                    light alone, to be added to the ray-traced map)
 * Several views in one go (read only if the key is there; 1 to
 * CMI_GPU_MAX_VIEWS):
 *   EmissionImages:number of views               1
 *   EmissionSkyMaps:number of observers          1
 * View 0 is described by the keys above. View k >= 1 is described by the
 * same keys with " k" appended: "view theta 1" and "view phi 1" (required),
 * "anchor x 1", "anchor y 1", "sides x 1", "sides y 1" (a missing one takes
 * view 0's value if view 0 names one, the bounding rectangle of view k's own
 * projection otherwise); "observer position 1" (required), "frame pole 1",
 * "frame zero longitude 1" and "exclusion radius 1" (a missing one takes
 * observer 0's). Resolution, window, dust, packets and seed are shared. View
 * 0's files keep their names; view k's carry "_view<k>" after the line's
 * name: <prefix>_<LineName>_view1.dat, <prefix>_<LineName>_view1_scattered_I.
 * The ray-traced maps of the further views are further calls of the same
 * renderer; with scattering all views are filled by one Monte Carlo run per
 * line (cmi_gpu_set_ccd_images, cmi_gpu_set_sky_cameras), so they share its
 * noise.
 * Spectral cubes (read only if "velocity channels" is there):
 *   EmissionImages:velocity channels             the number of channels
 *   EmissionImages:velocity minimum / velocity maximum   required, velocities
 *   EmissionImages:turbulent velocity dispersion 0. m s^-1
 *   EmissionImages:velocity field type           Static, or one of
 *     SolidBodyRotation: "angular velocity" (required, a frequency),
 *       "rotation axis" ([0, 0, 1]), "rotation centre" (the origin);
 *       v = omega axis x (r - centre)
 *     RadialExpansion: "expansion velocity" v0 and "expansion radius" r0
 *       (required), "expansion centre" (the origin); v = v0 (r - centre) / r0
 *     Snapshot: /PartType0/Velocities of the snapshot
 * Every flagged line that is the line of one ion is then also written as
 * <prefix>_<LineName>_cube.dat (_cube_view<k>.dat for view k >= 1): raw
 * doubles, [channel][ix][iy], next to its integrated image; the other flagged
 * entries keep their image and are named on stderr. PGM cannot hold a cube.
 * Sky cubes: the same keys in the EmissionSkyMaps: block,
 * "velocity channels" as the switch, with the block's own velocity field, and
 *   EmissionSkyMaps:observer velocity            [0., 0., 0.] m s^-1
 * ("observer velocity k" for observer k >= 1; observer 0's if absent). Every
 * flagged single-ion line is then also written as <prefix>_<LineName>_cube.dat
 * (_cube_view<k>.dat), raw doubles [channel][i][j], next to its map.
 * Scattered-light cubes: "scattered cubes: true" in either
 * block (default false; looked at like "scattering", so a file without it
 * has the used-values it had) needs "scattering: true" and "velocity
 * channels" of that block. Every flagged single-ion line's Monte Carlo run
 * then also fills a velocity cube per view, written as
 * <prefix>_<LineName>_scattered_cube_I / _Q / _U (_view<k> before
 * _scattered): raw doubles [channel][ix][iy] in the unit of the ray-traced
 * cube, with the block's velocity field, turbulent dispersion and observer
 * velocities.
 * Radio continuum (read only if "continuum frequencies" is
 * there, in either block):
 *   EmissionImages:continuum frequencies         N, the number of frequencies
 *   EmissionImages:continuum frequency minimum / continuum frequency maximum
 *                    required, frequencies (wavelengths and photon energies
 *                    convert); nu_f = nu_min * pow(nu_max / nu_min, f / (N -
 *                    1)), N == 1 uses the minimum
 *   EmissionImages:continuum background temperature   0. K: bg_f = B_nu(T_bg)
 * The thermal free-free emission of the cells with its own absorption is
 * then written as <prefix>_continuum.dat (_continuum_view<k>.dat for view or
 * observer k >= 1), raw doubles [f][ix][iy] in W m^-2 Hz^-1 sr^-1, and the
 * frequencies as <prefix>_continuum_frequencies.txt, one line "nu bg" per
 * frequency with 17 significant digits. Needs type BinaryArray.
 * H I cubes (read only with "HI cube: true", in either block,
 * which needs the block's "velocity channels", "velocity minimum" and
 * "velocity maximum"; the turbulent dispersion, the velocity field and the
 * observer velocities are the block's):
 *   EmissionImages:HI spin temperature type      Kinetic (the cells'
 *                    temperature) or Fixed
 *   EmissionImages:HI spin temperature           required for Fixed, > 0
 *   EmissionImages:HI free-free continuum        true: the ionized gas's
 *                    free-free emission and absorption at 1420 MHz
 *   EmissionImages:HI background temperature     0. K: B_nu(T_bg) behind the
 *                    box in every channel
 * The 21-cm line of the neutral gas with its own absorption is then written
 * as <prefix>_HI_cube.dat (_HI_cube_view<k>.dat), raw doubles [channel][ix]
 * [iy] in W m^-2 Hz^-1 sr^-1. Needs type BinaryArray.
 * Lyman alpha (read only with "Lyman alpha: true" in
 * EmissionImages, which needs type BinaryArray and the block's "velocity
 * channels", "velocity minimum" and "velocity maximum"; EmissionSkyMaps
 * refuses the key): packets from the cells' recombinations scatter off the
 * snapshot's own H I and off the block's dust, with the block's "number of
 * packets", "random seed", "turbulent velocity dispersion", velocity field,
 * dust keys and views, and
 *   EmissionImages:Lyman alpha core skipping          0. (x_crit)
 *   EmissionImages:Lyman alpha maximum scatterings    100000000
 * Written as <prefix>_LymanAlpha_image.dat and <prefix>_LymanAlpha_cube.dat
 * (_view<k> appended for view k >= 1), raw doubles [ix][iy] and [channel][ix]
 * [iy] in the unit of the scattered-light images and cubes.
 * Lyman-alpha radiation field (both keys are read only in
 * EmissionImages and only with "Lyman alpha: true"):
 *   EmissionImages:Lyman alpha radiation field   false: true writes the field
 *                    the run leaves in the cells as <prefix>_LymanAlpha_field
 *                    .dat, raw doubles [5][nx][ny][nz]: the energy density in
 *                    J m^-3, the scattering rate per H I atom in s^-1, the
 *                    force density x, y, z in N m^-3
 *   EmissionImages:HI Lyman alpha coupling       false (read only if the block
 *                    has "HI cube: true" as well; it implies the field): the
 *                    Lyman-alpha run comes first, and the H I cube is rendered
 *                    with the spin temperature that the run's scattering rate
 *                    and the cells' collisions give against "HI background
 *                    temperature" (Wouthuysen-Field coupling), written as
 *                    <prefix>_HI_spin_temperature.dat, raw doubles [nx][ny]
 *                    [nz] in K. Refused with "Lyman alpha core skipping" > 0
 *                    (the skipped scatterings are missing from the rate), with
 *                    "HI spin temperature type: Fixed" and with a background
 *                    temperature of 0. The H I cube of EmissionSkyMaps is not
 *                    coupled: it keeps its own spin temperature type.
 * Absorption spectra: an "AbsorptionSpectra:" block gives
 * the optical depths and column densities of resonance lines of the
 * snapshot's ions along sightlines from an observer; its keys and files stand
 * at AbsorptionSettings below. It needs no flagged emission line.
 * For the images and maps the cells go on the snapshot's real grid: the box
 * from /Parameters (SimulationBox:anchor, sides), each cell where its row of
 * /PartType0/Coordinates puts it (the box anchor is the origin in the file;
 * task-based snapshots are stored subgrid after subgrid). Without a block
 * nothing of it is read and the mode's files are what they were.
 */
#ifndef CMI_EMISSIONSETTINGS_HPP
#define CMI_EMISSIONSETTINGS_HPP

#include "GpuIonizationSimulation.hpp"
#include "ImageWriter.hpp"

#include <cstdio>
#include <iostream>

namespace cmi {
namespace emission {

/* the spectral cube keys of a block, "EmissionImages" or "EmissionSkyMaps"
 * (read only if the block has "velocity channels") */
struct CubeSettings {
  bool cubes = false;
  long long nchan = 0;
  double vmin = 0., vmax = 0., sigma_turb = 0.;
  std::string velocity_field = "Static";
  double angular_velocity = 0., expansion_velocity = 0.,
         expansion_radius = 1.;
  std::array<double, 3> rotation_axis = {0., 0., 1.},
                        field_centre = {0., 0., 0.};

  void read_cubes(ParameterFile &params, const std::string &block,
                  const std::string &type) {
    if (!params.has_value(block + ":velocity channels"))
      return;
    cubes = true;
    nchan = params.get_integer(block + ":velocity channels", 1);
    if (nchan < 1)
      throw ParameterError(block + ":velocity channels must be at "
                           "least 1");
    if (type != "BinaryArray")
      throw ParameterError(block + ":velocity channels needs type "
                           "BinaryArray: a cube is written as raw doubles");
    for (const char *name : {":velocity minimum", ":velocity maximum"})
      if (!params.has_value(block + name))
        throw ParameterError(block + name + " is required with " + block +
                             ":velocity channels");
    vmin = params.get_physical_value(
        QUANTITY_VELOCITY, block + ":velocity minimum", "0. m s^-1");
    vmax = params.get_physical_value(
        QUANTITY_VELOCITY, block + ":velocity maximum", "0. m s^-1");
    if (!(vmax > vmin) || !std::isfinite(vmax - vmin))
      throw ParameterError(block + ":velocity maximum must be above "
                           "velocity minimum, both finite");
    sigma_turb = params.get_physical_value(
        QUANTITY_VELOCITY, block + ":turbulent velocity dispersion",
        "0. m s^-1");
    if (!(sigma_turb >= 0.) || !std::isfinite(sigma_turb))
      throw ParameterError(block + ":turbulent velocity dispersion "
                           "must not be negative");
    velocity_field =
        params.get_string(block + ":velocity field type", "Static");
    const std::string origin = "[0. m, 0. m, 0. m]";
    if (velocity_field == "SolidBodyRotation") {
      if (!params.has_value(block + ":angular velocity"))
        throw ParameterError(block + ":angular velocity is required "
                             "for SolidBodyRotation");
      angular_velocity = params.get_physical_value(
          QUANTITY_FREQUENCY, block + ":angular velocity", "0. s^-1");
      rotation_axis = params.get_double_vector(
          block + ":rotation axis", {0., 0., 1.});
      double norm = 0.;
      for (int a = 0; a < 3; ++a)
        norm += rotation_axis[a] * rotation_axis[a];
      norm = std::sqrt(norm);
      if (!(norm > 0.) || !std::isfinite(norm))
        throw ParameterError(block + ":rotation axis must be a "
                             "finite vector that is not zero");
      for (int a = 0; a < 3; ++a)
        rotation_axis[a] /= norm;
      field_centre = params.get_physical_vector(
          QUANTITY_LENGTH, block + ":rotation centre", origin);
    } else if (velocity_field == "RadialExpansion") {
      for (const char *name : {":expansion velocity", ":expansion radius"})
        if (!params.has_value(block + name))
          throw ParameterError(block + name +
                               " is required for RadialExpansion");
      expansion_velocity = params.get_physical_value(
          QUANTITY_VELOCITY, block + ":expansion velocity",
          "0. m s^-1");
      expansion_radius = params.get_physical_value(
          QUANTITY_LENGTH, block + ":expansion radius", "1. m");
      if (!(expansion_radius > 0.))
        throw ParameterError(block + ":expansion radius must be "
                             "positive");
      field_centre = params.get_physical_vector(
          QUANTITY_LENGTH, block + ":expansion centre", origin);
    } else if (velocity_field != "Static" && velocity_field != "Snapshot") {
      throw ParameterError(
          "Unknown " + block + ":velocity field type \"" + velocity_field +
          "\" (Static, SolidBodyRotation, RadialExpansion or Snapshot)");
    }
  }

  /* the radio continuum keys of a block (read only if the block has
   * "continuum frequencies") */
  bool continuum = false;
  double continuum_background_temperature = 0.;
  std::vector<double> continuum_frequencies, continuum_background;

  void read_continuum(ParameterFile &params, const std::string &block,
                      const std::string &type) {
    if (!params.has_value(block + ":continuum frequencies"))
      return;
    continuum = true;
    const long long n =
        params.get_integer(block + ":continuum frequencies", 1);
    /* (the images of one call hold at most 2^28 values, checked against
     * the pixels where they are rendered; this bounds the ladder itself) */
    if (n < 1 || n > (1ll << 20))
      throw ParameterError(block + ":continuum frequencies must be between "
                           "1 and 2^20 (" + std::to_string(n) +
                           " asked for)");
    if (type != "BinaryArray")
      throw ParameterError(block + ":continuum frequencies needs type "
                           "BinaryArray: the images of all frequencies are "
                           "written as raw doubles");
    for (const char *name :
         {":continuum frequency minimum", ":continuum frequency maximum"})
      if (!params.has_value(block + name))
        throw ParameterError(block + name + " is required with " + block +
                             ":continuum frequencies");
    const double nu_min = params.get_physical_value(
        QUANTITY_FREQUENCY, block + ":continuum frequency minimum", "1. Hz");
    const double nu_max = params.get_physical_value(
        QUANTITY_FREQUENCY, block + ":continuum frequency maximum", "1. Hz");
    if (!(nu_min > 0.) || !std::isfinite(nu_min) || !(nu_max > 0.) ||
        !std::isfinite(nu_max))
      throw ParameterError(block + ":continuum frequency minimum and "
                           "maximum must be positive and finite");
    if (n > 1 && !(nu_max > nu_min))
      throw ParameterError(block + ":continuum frequency maximum must be "
                           "above continuum frequency minimum");
    continuum_background_temperature = params.get_physical_value(
        QUANTITY_TEMPERATURE, block + ":continuum background temperature",
        "0. K");
    if (!(continuum_background_temperature >= 0.) ||
        !std::isfinite(continuum_background_temperature))
      throw ParameterError(block + ":continuum background temperature must "
                           "not be negative");
    continuum_frequencies.resize((size_t)n);
    continuum_background.resize((size_t)n);
    for (long long f = 0; f < n; ++f) {
      const double nu =
          n == 1 ? nu_min
                 : nu_min * std::pow(nu_max / nu_min,
                                     (double)f / (double)(n - 1));
      continuum_frequencies[(size_t)f] = nu;
      const double T = continuum_background_temperature;
      continuum_background[(size_t)f] =
          T > 0. ? (2. * constants::planck * nu * nu * nu /
                    (constants::lightspeed * constants::lightspeed)) /
                       std::expm1((constants::planck * nu) /
                                  (constants::boltzmann * T))
                 : 0.;
    }
  }

  /* the 21-cm keys of a block (read only if the block has "HI cube: true",
   * looked at like "scattering") */
  bool hi_cube = false, hi_free_free = true;
  int32_t hi_spin_mode = 0; /* 0: the kinetic temperature, 1: one value */
  double hi_spin_temperature = 0., hi_background_temperature = 0.;

  void read_hi(ParameterFile &params, const std::string &block,
               const std::string &type) {
    if (!params.peek_bool(block + ":HI cube"))
      return;
    hi_cube = params.get_bool(block + ":HI cube", false);
    if (type != "BinaryArray")
      throw ParameterError(block + ":HI cube needs type BinaryArray: a cube "
                           "is written as raw doubles");
    if (!cubes)
      throw ParameterError(block + ":HI cube needs velocity channels, "
                           "velocity minimum and velocity maximum");
    const std::string kind =
        params.get_string(block + ":HI spin temperature type", "Kinetic");
    if (kind == "Fixed") {
      if (!params.has_value(block + ":HI spin temperature"))
        throw ParameterError(block + ":HI spin temperature is required with "
                             "HI spin temperature type Fixed");
      hi_spin_mode = 1;
      hi_spin_temperature = params.get_physical_value(
          QUANTITY_TEMPERATURE, block + ":HI spin temperature", "0. K");
      if (!(hi_spin_temperature > 0.) || !std::isfinite(hi_spin_temperature))
        throw ParameterError(block + ":HI spin temperature must be positive");
    } else if (kind != "Kinetic") {
      throw ParameterError("Unknown " + block +
                           ":HI spin temperature type \"" + kind +
                           "\" (Kinetic or Fixed)");
    }
    hi_free_free =
        params.get_bool(block + ":HI free-free continuum", true);
    hi_background_temperature = params.get_physical_value(
        QUANTITY_TEMPERATURE, block + ":HI background temperature", "0. K");
    if (!(hi_background_temperature >= 0.) ||
        !std::isfinite(hi_background_temperature))
      throw ParameterError(block + ":HI background temperature must not be "
                           "negative");
  }

  /* <name>.txt: one line "nu bg" per frequency. Returns the file's name. */
  std::string write_continuum_frequencies(const std::string &name) const {
    const std::string filename = name + ".txt";
    std::FILE *file = std::fopen(filename.c_str(), "w");
    if (!file)
      throw std::runtime_error("Could not write " + filename);
    for (size_t f = 0; f < continuum_frequencies.size(); ++f)
      std::fprintf(file, "%.17g %.17g\n", continuum_frequencies[f],
                   continuum_background[f]);
    std::fclose(file);
    return filename;
  }

  /* the velocity of the matter at r (not for Snapshot) */
  std::array<double, 3> velocity_at(const std::array<double, 3> &r) const {
    const double d[3] = {r[0] - field_centre[0], r[1] - field_centre[1],
                         r[2] - field_centre[2]};
    if (velocity_field == "SolidBodyRotation") {
      const std::array<double, 3> &w = rotation_axis;
      return {angular_velocity * (w[1] * d[2] - w[2] * d[1]),
              angular_velocity * (w[2] * d[0] - w[0] * d[2]),
              angular_velocity * (w[0] * d[1] - w[1] * d[0])};
    }
    if (velocity_field == "RadialExpansion") {
      const double scale = expansion_velocity / expansion_radius;
      return {scale * d[0], scale * d[1], scale * d[2]};
    }
    return {0., 0., 0.};
  }
};

/* what the EmissionImages: and EmissionSkyMaps: blocks share beyond the
 * cubes: the dust, where and how the files are written, and the scattered
 * light. Every key is read under the block's own name. */
struct ProductSettings : CubeSettings {
  const std::string block;
  double dust_cross_section = 0.;
  std::string type, prefix, folder;
  /* scattered light (the keys of read_scattering are read only if the block's
   * rule for them says so) */
  bool scattering = false;
  /* "scattered cubes": every flagged single-ion line's scattered light
   * also per velocity channel */
  bool scattered_cubes = false;
  long long npackets = 1000000, seed = 42;
  double albedo = 0., asymmetry = 0.5, polarisation = 0.;

  explicit ProductSettings(const char *name) : block(name) {}

  /* the dust cross section, "type", "filename prefix", "output folder" */
  void read_output(ParameterFile &params, const char *default_prefix) {
    dust_cross_section = params.get_physical_value(
        QUANTITY_SURFACE_AREA, block + ":dust cross section per hydrogen",
        "0. m^2");
    type = params.get_string(block + ":type", "BinaryArray");
    prefix = params.get_string(block + ":filename prefix", default_prefix);
    folder = params.get_string(block + ":output folder", ".");
    if (!is_image_type(type))
      throw ParameterError("Unknown " + block + ":type \"" + type +
                           "\" (BinaryArray or PGM)");
  }

  /* (after the checks of the block's geometry, where it always was) */
  void check_cross_section() const {
    if (!(dust_cross_section >= 0.))
      throw ParameterError(block + ":dust cross section per hydrogen must not "
                           "be negative");
  }

  /* (a key that is read shows in the used-values: the switch is looked at
   * with peek_bool, so a file without it, or with it false, has the
   * used-values it had, the switch included) */
  void read_scattered_cubes(ParameterFile &params) {
    if (!params.peek_bool(block + ":scattered cubes"))
      return;
    if (!params.peek_bool(block + ":scattering"))
      throw ParameterError(block + ":scattered cubes needs scattering: true");
    if (!cubes)
      throw ParameterError(block + ":scattered cubes needs velocity channels");
    scattered_cubes = params.get_bool(block + ":scattered cubes", false);
  }

  /* the switch itself (if it is on), the packets, the seed and the dust keys */
  void read_scattering(ParameterFile &params) {
    if (params.peek_bool(block + ":scattering"))
      scattering = params.get_bool(block + ":scattering", false);
    npackets = params.get_integer(block + ":number of packets", 1000000);
    seed = params.get_integer(block + ":random seed", 42);
    if (npackets <= 0)
      throw ParameterError(block + ":number of packets must be positive");
    if (seed < 0 || seed > 0xffffffffll)
      throw ParameterError(block + ":random seed must fit 32 bits");
    static const char *keys[3] = {":dust albedo", ":dust asymmetry",
                                  ":dust peak linear polarisation"};
    double *values[3] = {&albedo, &asymmetry, &polarisation};
    for (int k = 0; k < 3; ++k) {
      if (params.has_value(block + keys[k]))
        *values[k] = params.get_double(block + keys[k], *values[k]);
      else if (dust_cross_section > 0.)
        throw ParameterError(block + keys[k] +
                             " is required for scattering off dust with a "
                             "cross section above 0");
    }
    if (!(albedo >= 0. && albedo <= 1.))
      throw ParameterError(block + ":dust albedo must be in [0, 1]");
    if (!(asymmetry != 0. && std::fabs(asymmetry) < 1.))
      throw ParameterError(block + ":dust asymmetry must be non-zero and "
                           "inside (-1, 1)");
  }

  /* "number of views" / "number of observers", 1 without the key */
  long long read_count(ParameterFile &params, const std::string &key) const {
    const long long n =
        params.has_value(block + key) ? params.get_integer(block + key, 1) : 1;
    if (n < 1 || n > CMI_GPU_MAX_VIEWS)
      throw ParameterError(block + key + " must be 1.." +
                           std::to_string(CMI_GPU_MAX_VIEWS));
    return n;
  }

  /* <folder>/<prefix>_<product><kind><view tag><stokes>: view 0's files keep
   * their names, view k's carry "_view<k>" */
  std::string file_name(const std::string &product,
                        const std::string &kind = "", size_t view = 0,
                        const std::string &stokes = "") const {
    return folder + "/" + prefix + "_" + product + kind +
           (view ? "_view" + std::to_string(view) : std::string()) + stokes;
  }
};

/* the EmissionImages: block (read only if the file has one) */
struct ImageSettings : ProductSettings {
  long long nx = 200, ny = 200, supersample = 1;
  /* "Lyman alpha": the Monte Carlo Lyman-alpha image and cube of the
   * snapshot's own H I; it reads the packets, the seed and
   * the dust keys of the scattered light */
  bool lyman_alpha = false;
  /* "Lyman alpha radiation field", "HI Lyman alpha coupling" (DESIGN.md
   * 4.18): what the run leaves in the cells, and the H I cube with the spin
   * temperature it gives */
  bool lya_field = false, lya_coupling = false;
  double lya_core_skip = 0.;
  long long lya_max_scatter = 100000000;
  /* views[0] is read from the keys as they stand, views[k] from the keys
   * with " k" appended */
  struct View {
    double theta = 0., phi = 0.;
    bool have_anchor[2] = {false, false}, have_sides[2] = {false, false};
    double anchor[2] = {0., 0.}, sides[2] = {0., 0.};
  };
  std::vector<View> views;

  ImageSettings() : ProductSettings("EmissionImages") {}

  /* "anchor x<n>" ... "sides y<n>" where the file has them */
  void read_rectangle(ParameterFile &params, const std::string &n, View &v) {
    static const char *axis[2] = {"x", "y"};
    for (int a = 0; a < 2; ++a) {
      const std::string ka = block + ":anchor " + axis[a] + n;
      const std::string ks = block + ":sides " + axis[a] + n;
      if (params.has_value(ka)) {
        v.have_anchor[a] = true;
        v.anchor[a] = params.get_physical_value(QUANTITY_LENGTH, ka, "0. m");
      }
      if (params.has_value(ks)) {
        v.have_sides[a] = true;
        v.sides[a] = params.get_physical_value(QUANTITY_LENGTH, ks, "1. m");
      }
    }
  }
  static void check_sides(const View &v) {
    for (int a = 0; a < 2; ++a)
      if (v.have_sides[a] && !(v.sides[a] > 0.))
        throw ParameterError("EmissionImages: the image sides must be "
                             "positive");
  }

  /* views 1 .. "number of views" - 1 (a missing anchor or side is view 0's) */
  void read_views(ParameterFile &params) {
    const long long nviews = read_count(params, ":number of views");
    for (long long k = 1; k < nviews; ++k) {
      const std::string n = " " + std::to_string(k);
      View v = views[0];
      const std::string kt = "EmissionImages:view theta" + n;
      const std::string kp = "EmissionImages:view phi" + n;
      if (!params.has_value(kt))
        throw ParameterError(kt + " is required");
      if (!params.has_value(kp))
        throw ParameterError(kp + " is required");
      v.theta = params.get_physical_value(QUANTITY_ANGLE, kt, "0. degrees");
      v.phi = params.get_physical_value(QUANTITY_ANGLE, kp, "0. degrees");
      read_rectangle(params, n, v);
      check_sides(v);
      views.push_back(v);
    }
  }

  /* (looked at like "scattered cubes") */
  void read_lyman_alpha(ParameterFile &params) {
    if (!params.peek_bool("EmissionImages:Lyman alpha"))
      return;
    lyman_alpha = params.get_bool("EmissionImages:Lyman alpha", false);
    if (type != "BinaryArray")
      throw ParameterError("EmissionImages:Lyman alpha needs type "
                           "BinaryArray: a cube is written as raw doubles");
    if (!cubes)
      throw ParameterError("EmissionImages:Lyman alpha needs velocity "
                           "channels, velocity minimum and velocity "
                           "maximum");
    lya_core_skip =
        params.get_double("EmissionImages:Lyman alpha core skipping", 0.);
    if (!(lya_core_skip >= 0.) || !std::isfinite(lya_core_skip))
      throw ParameterError("EmissionImages:Lyman alpha core skipping must "
                           "not be negative");
    lya_max_scatter = params.get_integer(
        "EmissionImages:Lyman alpha maximum scatterings", 100000000);
    if (lya_max_scatter < 1 || lya_max_scatter > 100000000)
      throw ParameterError("EmissionImages:Lyman alpha maximum "
                           "scatterings must be 1..100000000");
    if (params.peek_bool("EmissionImages:Lyman alpha radiation field"))
      lya_field = params.get_bool(
          "EmissionImages:Lyman alpha radiation field", false);
    if (hi_cube &&
        params.peek_bool("EmissionImages:HI Lyman alpha coupling")) {
      lya_coupling =
          params.get_bool("EmissionImages:HI Lyman alpha coupling", false);
      if (lya_core_skip > 0.)
        throw ParameterError(
            "EmissionImages:HI Lyman alpha coupling needs "
            "EmissionImages:Lyman alpha core skipping 0: the skipped "
            "scatterings are missing from the scattering rate");
      if (hi_spin_mode != 0)
        throw ParameterError(
            "EmissionImages:HI Lyman alpha coupling computes the spin "
            "temperature: EmissionImages:HI spin temperature type must "
            "not be Fixed");
      if (!(hi_background_temperature > 0.))
        throw ParameterError(
            "EmissionImages:HI Lyman alpha coupling needs a positive "
            "EmissionImages:HI background temperature");
      lya_field = true;
    }
  }

  void read(ParameterFile &params) {
    views.assign(1, View());
    views[0].theta = params.get_physical_value(
        QUANTITY_ANGLE, "EmissionImages:view theta", "0. degrees");
    views[0].phi = params.get_physical_value(
        QUANTITY_ANGLE, "EmissionImages:view phi", "0. degrees");
    nx = params.get_integer("EmissionImages:image width", 200);
    ny = params.get_integer("EmissionImages:image height", 200);
    read_rectangle(params, "", views[0]);
    supersample = params.get_integer("EmissionImages:supersampling", 1);
    read_output(params, "line_image");
    if (nx <= 0 || ny <= 0 || nx * ny > (1ll << 28))
      throw ParameterError("EmissionImages: image width and height must be "
                           "positive, 2^28 pixels at most (" +
                           std::to_string(nx) + " x " + std::to_string(ny) +
                           " asked for)");
    if (supersample < 1 || supersample > 8)
      throw ParameterError("EmissionImages:supersampling must be 1..8");
    check_cross_section();
    check_sides(views[0]);
    read_views(params);
    read_cubes(params, block, type);
    read_continuum(params, block, type);
    read_hi(params, block, type);
    read_scattered_cubes(params);
    read_lyman_alpha(params);
    /* the Lyman-alpha run shoots the packets of these keys through the dust
     * of these keys */
    if (lyman_alpha || params.peek_bool("EmissionImages:scattering"))
      read_scattering(params);
  }
};

/* the EmissionSkyMaps: block (read only if the file has one) */
struct SkyMapSettings : ProductSettings {
  long long nlon = 360, nlat = 180;
  std::array<double, 2> lon = {0., 0.}, lat = {0., 0.};
  bool direct_light = true;   /* read with the scattering keys */
  double camera_lon_max = 0.; /* min(lon[1], lon[0] + 2 pi) */
  /* the observers as the engine takes them, [observer][3], [9], [1], [3]:
   * observer 0 from the keys as they stand, observer k from the keys with
   * " k" appended; the velocities are read with the cubes, the radii with
   * the scattering keys */
  std::vector<double> positions, frames, velocities, exclusion_radii;

  SkyMapSettings() : ProductSettings("EmissionSkyMaps") {}

  /* Gram-Schmidt: e_3 = the pole, e_1 = the zero of longitude made
   * perpendicular to it, e_2 = e_3 x e_1 */
  static void make_frame(const std::array<double, 3> &pole,
                         const std::array<double, 3> &zero,
                         const std::string &n, double frame[9]) {
    double e3[3], e1[3];
    double norm = std::sqrt(pole[0] * pole[0] + pole[1] * pole[1] +
                            pole[2] * pole[2]);
    const double zero_norm = std::sqrt(zero[0] * zero[0] + zero[1] * zero[1] +
                                       zero[2] * zero[2]);
    if (!(norm > 0.) || !std::isfinite(norm) || !(zero_norm > 0.) ||
        !std::isfinite(zero_norm))
      throw ParameterError("EmissionSkyMaps:frame pole" + n +
                           " and frame zero longitude" + n +
                           " must be finite vectors, not zero");
    for (int a = 0; a < 3; ++a)
      e3[a] = pole[a] / norm;
    const double along = zero[0] * e3[0] + zero[1] * e3[1] + zero[2] * e3[2];
    for (int a = 0; a < 3; ++a)
      e1[a] = zero[a] - along * e3[a];
    norm = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    if (!(norm > 1.e-8 * zero_norm))
      throw ParameterError("EmissionSkyMaps:frame pole" + n +
                           " and frame zero longitude" + n +
                           " are parallel");
    for (int a = 0; a < 3; ++a)
      e1[a] /= norm;
    const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1],
                          e3[2] * e1[0] - e3[0] * e1[2],
                          e3[0] * e1[1] - e3[1] * e1[0]};
    for (int a = 0; a < 3; ++a) {
      frame[a] = e1[a];
      frame[3 + a] = e2[a];
      frame[6 + a] = e3[a];
    }
  }

  /* observers 1 .. "number of observers" - 1: positions and frames */
  void read_observers(ParameterFile &params,
                      const std::array<double, 3> &pole,
                      const std::array<double, 3> &zero) {
    const long long nobservers = read_count(params, ":number of observers");
    for (long long k = 1; k < nobservers; ++k) {
      const std::string n = " " + std::to_string(k);
      const std::string key = "EmissionSkyMaps:observer position" + n;
      if (!params.has_value(key))
        throw ParameterError(key + " is required");
      const std::array<double, 3> position =
          params.get_physical_vector(QUANTITY_LENGTH, key, "");
      for (int a = 0; a < 3; ++a)
        if (!std::isfinite(position[a]))
          throw ParameterError(key + " must be finite");
      positions.insert(positions.end(), position.begin(), position.end());
      const std::string kpole = "EmissionSkyMaps:frame pole" + n;
      const std::string kzero = "EmissionSkyMaps:frame zero longitude" + n;
      const std::array<double, 3> p =
          params.has_value(kpole) ? params.get_double_vector(kpole, pole)
                                  : pole;
      const std::array<double, 3> z =
          params.has_value(kzero) ? params.get_double_vector(kzero, zero)
                                  : zero;
      frames.resize(frames.size() + 9);
      make_frame(p, z, n, &frames[9 * k]);
    }
    velocities.assign(3 * nobservers, 0.);
    exclusion_radii.assign(nobservers, 0.);
  }

  /* sky cubes: "observer velocity", and "observer velocity k" for observer
   * k >= 1 (observer 0's where the key is absent) */
  void read_observer_velocities(ParameterFile &params) {
    for (size_t k = 0; k < exclusion_radii.size(); ++k) {
      const std::string key = "EmissionSkyMaps:observer velocity" +
                              (k ? " " + std::to_string(k) : std::string());
      if (k == 0 || params.has_value(key)) {
        const std::array<double, 3> velocity = params.get_physical_vector(
            QUANTITY_VELOCITY, key, "[0. m s^-1, 0. m s^-1, 0. m s^-1]");
        std::copy(velocity.begin(), velocity.end(), &velocities[3 * k]);
      } else {
        std::copy(&velocities[0], &velocities[3], &velocities[3 * k]);
      }
      for (int a = 0; a < 3; ++a)
        if (!std::isfinite(velocities[3 * k + a]))
          throw ParameterError(key + " must be finite");
    }
  }

  /* "exclusion radius", and "exclusion radius k" for observer k >= 1
   * (observer 0's where the key is absent) */
  void read_exclusion_radii(ParameterFile &params) {
    if (!params.has_value("EmissionSkyMaps:exclusion radius"))
      throw ParameterError("EmissionSkyMaps:exclusion radius is required "
                           "for scattering");
    const double radius = params.get_physical_value(
        QUANTITY_LENGTH, "EmissionSkyMaps:exclusion radius", "0. m");
    if (!(radius >= 0.) || !std::isfinite(radius))
      throw ParameterError("EmissionSkyMaps:exclusion radius must be "
                           "finite and not negative");
    exclusion_radii[0] = radius;
    for (size_t k = 1; k < exclusion_radii.size(); ++k) {
      const std::string key =
          "EmissionSkyMaps:exclusion radius " + std::to_string(k);
      double r = radius;
      if (params.has_value(key))
        r = params.get_physical_value(QUANTITY_LENGTH, key, "0. m");
      if (!(r >= 0.) || !std::isfinite(r))
        throw ParameterError(key + " must be finite and not negative");
      exclusion_radii[k] = r;
    }
  }

  void read(ParameterFile &params) {
    if (!params.has_value("EmissionSkyMaps:observer position"))
      throw ParameterError("EmissionSkyMaps:observer position is required");
    const std::array<double, 3> position = params.get_physical_vector(
        QUANTITY_LENGTH, "EmissionSkyMaps:observer position", "");
    positions.assign(position.begin(), position.end());
    nlon = params.get_integer("EmissionSkyMaps:number of longitude pixels",
                              360);
    nlat = params.get_integer("EmissionSkyMaps:number of latitude pixels",
                              180);
    lon = params.get_physical_pair(QUANTITY_ANGLE,
                                   "EmissionSkyMaps:longitude range",
                                   "[-180. degrees, 180. degrees]");
    lat = params.get_physical_pair(QUANTITY_ANGLE,
                                   "EmissionSkyMaps:latitude range",
                                   "[-90. degrees, 90. degrees]");
    const std::array<double, 3> pole = params.get_double_vector(
        "EmissionSkyMaps:frame pole", {0., 0., 1.});
    const std::array<double, 3> zero = params.get_double_vector(
        "EmissionSkyMaps:frame zero longitude", {1., 0., 0.});
    read_output(params, "sky_map");
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(position[a]))
        throw ParameterError("EmissionSkyMaps:observer position must be "
                             "finite");
    if (nlon <= 0 || nlat <= 0 || nlon * nlat > (1ll << 28))
      throw ParameterError(
          "EmissionSkyMaps: the numbers of longitude pixels and latitude "
          "pixels must be positive, 2^28 pixels at most (" +
          std::to_string(nlon) + " x " + std::to_string(nlat) +
          " asked for)");
    if (!std::isfinite(lon[0]) || !std::isfinite(lon[1]) ||
        !(lon[0] < lon[1]))
      throw ParameterError("EmissionSkyMaps:longitude range must be "
                           "increasing");
    /* (90 degrees converted to radians may overshoot pi / 2 by an ulp) */
    const double half_pi = 0.5 * M_PI;
    for (int k = 0; k < 2; ++k)
      if (std::fabs(std::fabs(lat[k]) - half_pi) < 1.e-12)
        lat[k] = lat[k] < 0. ? -half_pi : half_pi;
    if (!(lat[0] < lat[1]) || !(lat[0] >= -half_pi) || !(lat[1] <= half_pi))
      throw ParameterError("EmissionSkyMaps:latitude range must be "
                           "increasing and within [-90, 90] degrees");
    check_cross_section();
    frames.assign(9, 0.);
    make_frame(pole, zero, "", &frames[0]);
    read_observers(params, pole, zero);
    read_cubes(params, block, type);
    if (cubes)
      read_observer_velocities(params);
    read_continuum(params, block, type);
    read_hi(params, block, type);
    read_scattered_cubes(params);
    if (params.peek_bool("EmissionSkyMaps:Lyman alpha"))
      throw ParameterError("EmissionSkyMaps:Lyman alpha is not supported: "
                           "the Lyman-alpha transfer serves the parallel "
                           "cameras of EmissionImages only");
    if (!params.peek_bool("EmissionSkyMaps:scattering"))
      return;
    read_scattering(params);
    read_exclusion_radii(params);
    direct_light = params.get_bool("EmissionSkyMaps:direct light", true);
    /* (360 degrees converted to radians may overshoot 2 pi by an ulp) */
    if (lon[1] - lon[0] > 2. * M_PI * (1. + 1.e-12))
      throw ParameterError("EmissionSkyMaps:longitude range must not be "
                           "wider than 360 degrees with scattering");
    /* the camera alone gets the clamped end: the ray-traced map keeps the
     * range as converted, whatever the switch */
    camera_lon_max = std::min(lon[1], lon[0] + 2. * M_PI);
  }
};

/* a resonance line of one of the engine's ions: the table of
 * cmacionize_amd/engine.py (ABSORPTION_LINES has the sources), the same
 * literals; tests/test_absorption_host.py holds the two together */
struct AbsorptionLine {
  const char *name;
  int32_t ion;
  double weight, wavelength, f, gamma;
  /* absorption_line_constants of engine.py, operation for operation */
  double S() const {
    return 1.602176634e-19 * 1.602176634e-19 * f * wavelength /
           (4. * 8.8541878128e-12 * 9.1093837015e-31 * 299792458.);
  }
  double g() const { return gamma * wavelength / (4. * M_PI); }
};
inline const AbsorptionLine *absorption_line(const std::string &name) {
  static const AbsorptionLine table[] = {
      {"HI_1215", 0, 1.00794, 1215.67e-10, 0.4164, 6.265e8},
      {"HeI_584", 1, 4.002602, 584.334e-10, 0.2763, 1.799e9},
      {"CII_1334", 2, 12.0107, 1334.532e-10, 0.1278, 2.88e8},
      {"CIII_977", 3, 12.0107, 977.020e-10, 0.7570, 1.767e9},
      {"NI_1199", 4, 14.0067, 1199.550e-10, 0.1320, 4.07e8},
      {"NII_1083", 5, 14.0067, 1083.994e-10, 0.1110, 3.74e8},
      {"NIII_989", 6, 14.0067, 989.799e-10, 0.1230, 5.00e8},
      {"OI_1302", 7, 15.9994, 1302.168e-10, 0.0480, 5.65e8},
      {"OII_834", 8, 15.9994, 834.466e-10, 0.1320, 8.60e8},
      {"NeI_735", 9, 20.1797, 735.896e-10, 0.1590, 6.11e8},
      {"NeII_460", 10, 20.1797, 460.728e-10, 0.0900, 7.00e9},
      {"SII_1259", 11, 32.065, 1259.518e-10, 0.0166, 4.65e7},
      {"SIII_1190", 12, 32.065, 1190.203e-10, 0.0237, 6.70e7},
      {"SIV_1062", 13, 32.065, 1062.664e-10, 0.0494, 1.60e8}};
  for (const AbsorptionLine &line : table)
    if (name == line.name)
      return &line;
  return nullptr;
}

/* the AbsorptionSpectra: block (read only if the file has one; DESIGN.md
 * 4.19): sightlines from an observer, each along a direction to the edge of
 * the box or towards a target at a finite distance, and the optical depths
 * of the named lines along them.
 *   AbsorptionSpectra:observer position        required, a vector of lengths
 *   AbsorptionSpectra:observer velocity        [0., 0., 0.] m s^-1
 *   AbsorptionSpectra:number of sightlines     1
 *   AbsorptionSpectra:sightline direction k    a vector, normalised here, or
 *   AbsorptionSpectra:target position k        a vector of lengths: the
 *                    direction towards it and L = its distance; exactly one
 *                    of the two for every k = 0 .. K - 1
 *   AbsorptionSpectra:lines                    required, [names] of the table
 *   AbsorptionSpectra:velocity channels / velocity minimum / velocity
 *                    maximum                   required
 *   AbsorptionSpectra:turbulent velocity dispersion / velocity field type
 *                    and its keys              as in EmissionImages
 *   AbsorptionSpectra:filename prefix / output folder   absorption / .
 * Written: <prefix>_absorption_tau.dat, raw doubles [ray][line][channel],
 * and <prefix>_absorption_columns.txt, one row "ray line N W" per ray and
 * line: the column density in m^-2 and the equivalent width in m. */
struct AbsorptionSettings : CubeSettings {
  std::array<double, 3> position = {0., 0., 0.}, velocity = {0., 0., 0.};
  std::vector<double> origins, directions, lengths;
  std::vector<const AbsorptionLine *> lines;
  std::string prefix, folder;

  void read(ParameterFile &params) {
    const std::string block = "AbsorptionSpectra";
    if (!params.has_value(block + ":observer position"))
      throw ParameterError(block + ":observer position is required");
    position = params.get_physical_vector(
        QUANTITY_LENGTH, block + ":observer position", "");
    velocity = params.get_physical_vector(
        QUANTITY_VELOCITY, block + ":observer velocity",
        "[0. m s^-1, 0. m s^-1, 0. m s^-1]");
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(position[a]) || !std::isfinite(velocity[a]))
        throw ParameterError(block + ":observer position and velocity must "
                             "be finite");
    const long long nrays =
        params.get_integer(block + ":number of sightlines", 1);
    if (nrays < 1 || nrays > (1ll << 20))
      throw ParameterError(block + ":number of sightlines must be between "
                           "1 and 2^20");
    for (long long k = 0; k < nrays; ++k) {
      const std::string kd =
          block + ":sightline direction " + std::to_string(k);
      const std::string kt = block + ":target position " + std::to_string(k);
      const bool has_d = params.has_value(kd), has_t = params.has_value(kt);
      if (has_d && has_t)
        throw ParameterError(kd + " and " + kt + " are both given: a "
                             "sightline has a direction or a target");
      if (!has_d && !has_t)
        throw ParameterError("one of " + kd + " and " + kt +
                             " is required");
      std::array<double, 3> d;
      if (has_d) {
        d = params.get_double_vector(kd, {0., 0., 0.});
      } else {
        const std::array<double, 3> target =
            params.get_physical_vector(QUANTITY_LENGTH, kt, "");
        for (int a = 0; a < 3; ++a)
          d[a] = target[a] - position[a];
      }
      const double norm = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      if (!(norm > 0.) || !std::isfinite(norm))
        throw ParameterError((has_d ? kd : kt) + " must be a finite vector "
                             "that is not zero" +
                             (has_d ? "" : ", away from the observer"));
      for (int a = 0; a < 3; ++a) {
        origins.push_back(position[a]);
        directions.push_back(d[a] / norm);
      }
      lengths.push_back(has_d ? HUGE_VAL : norm);
    }
    if (!params.has_value(block + ":lines"))
      throw ParameterError(block + ":lines is required");
    std::string names = params.get_string(block + ":lines", "");
    for (char &c : names)
      if (c == '[' || c == ']' || c == ',')
        c = ' ';
    std::istringstream words(names);
    for (std::string name; words >> name;) {
      const AbsorptionLine *line = absorption_line(name);
      if (!line)
        throw ParameterError("Unknown " + block + ":lines entry \"" + name +
                             "\"");
      lines.push_back(line);
    }
    if (lines.empty() || lines.size() > 16)
      throw ParameterError(block + ":lines must name between 1 and 16 "
                           "lines");
    if (!params.has_value(block + ":velocity channels"))
      throw ParameterError(block + ":velocity channels is required");
    read_cubes(params, block, "BinaryArray");
    if ((double)nrays * (double)lines.size() * (double)nchan >
        (double)(1ll << 28))
      throw ParameterError(block + ": more than 2^28 optical depths in one "
                           "call");
    prefix = params.get_string(block + ":filename prefix", "absorption");
    folder = params.get_string(block + ":output folder", ".");
  }

  /* what --describe prints */
  void describe(std::ostream &os) const {
    char text[64];
    auto number = [&text](double x) {
      std::snprintf(text, sizeof text, "%.17g", x);
      return std::string(std::isfinite(x) ? text : "null");
    };
    os << "{\"AbsorptionSpectra\": {\"observer position\": ["
       << number(position[0]) << ", " << number(position[1]) << ", "
       << number(position[2]) << "], \"observer velocity\": ["
       << number(velocity[0]) << ", " << number(velocity[1]) << ", "
       << number(velocity[2]) << "],\n  \"sightlines\": [";
    for (size_t k = 0; k < lengths.size(); ++k)
      os << (k ? ",\n    " : "\n    ") << "{\"direction\": ["
         << number(directions[3 * k]) << ", "
         << number(directions[3 * k + 1]) << ", "
         << number(directions[3 * k + 2])
         << "], \"length\": " << number(lengths[k]) << "}";
    os << "],\n  \"lines\": [";
    for (size_t l = 0; l < lines.size(); ++l)
      os << (l ? ",\n    " : "\n    ") << "{\"name\": \"" << lines[l]->name
         << "\", \"ion\": " << lines[l]->ion
         << ", \"weight\": " << number(lines[l]->weight)
         << ", \"wavelength\": " << number(lines[l]->wavelength)
         << ", \"S\": " << number(lines[l]->S())
         << ", \"g\": " << number(lines[l]->g()) << "}";
    os << "],\n  \"velocity channels\": " << nchan
       << ", \"velocity minimum\": " << number(vmin)
       << ", \"velocity maximum\": " << number(vmax)
       << ", \"turbulent velocity dispersion\": " << number(sigma_turb)
       << ", \"velocity field type\": \"" << velocity_field
       << "\",\n  \"filename prefix\": \"" << prefix
       << "\", \"output folder\": \"" << folder << "\"}}" << std::endl;
  }
};

/* the flagged lines of "EmissivityValues:" and the blocks the file has */
struct Settings {
  std::vector<int32_t> lines;
  bool do_images = false, do_sky = false, do_absorption = false;
  ImageSettings img;
  SkyMapSettings sky;
  AbsorptionSettings absorption;

  static const char *line_name(int32_t line) {
    return GpuIonizationSimulation::emission_line_name(line);
  }

  explicit Settings(ParameterFile &params) {
    for (int32_t i = 0; i < CMI_GPU_NUMBER_OF_EMISSIONLINES; ++i)
      if (params.get_bool(std::string("EmissivityValues:") + line_name(i),
                          false))
        lines.push_back(i);
    if ((do_images = params.has_block("EmissionImages")))
      img.read(params);
    if ((do_sky = params.has_block("EmissionSkyMaps")))
      sky.read(params);
    if ((do_absorption = params.has_block("AbsorptionSpectra")))
      absorption.read(params);
  }
};

} // namespace emission
} // namespace cmi

#endif
