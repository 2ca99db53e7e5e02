/*
 * EmissivityCalculationSimulation.hpp - the reference's emission mode
 * (`CMacIonize --emission --params lines.param --file snapshot.hdf5`,
 * src/EmissivityCalculationSimulation.cpp:58-299) on the GPU engine: reads the
 * state of a snapshot, computes the emission lines flagged in
 * "EmissivityValues:<name>" on the device (cmi_gpu_compute_emissivities) and
 * adds them to the snapshot as datasets /PartType0/<name>.
 *
 * The reference appends the datasets through libhdf5; here the file is read
 * with Hdf5Reader and written anew with Hdf5Writer (same groups, attributes
 * and datasets, plus the lines), then moved over the original.
 *
 * Beyond the reference: if - and only if - the parameter file has an
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
#ifndef CMI_EMISSIVITYCALCULATIONSIMULATION_HPP
#define CMI_EMISSIVITYCALCULATIONSIMULATION_HPP

#include "GpuIonizationSimulation.hpp"
#include "Hdf5Reader.hpp"
#include "ImageWriter.hpp"

#include <cstdio>
#include <iostream>

namespace cmi {

class EmissivityCalculationSimulation {
  static void check(int rc, const char *what) {
    if (rc != CMI_GPU_OK)
      throw std::runtime_error(std::string(what) + ": " +
                               cmi_gpu_last_error());
  }

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

  /* the EmissionImages: block (read only if the file has one) */
  struct ImageSettings : CubeSettings {
    double theta = 0., phi = 0.;
    long long nx = 200, ny = 200, supersample = 1;
    bool have_anchor[2] = {false, false}, have_sides[2] = {false, false};
    double anchor[2] = {0., 0.}, sides[2] = {0., 0.};
    double dust_cross_section = 0.;
    std::string type, prefix, folder;
    /* scattered light (the keys below are read only if scattering is set) */
    bool scattering = false;
    /* "scattered cubes": every flagged single-ion line's scattered light
     * also per velocity channel */
    bool scattered_cubes = false;
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
    long long npackets = 1000000, seed = 42;
    double albedo = 0., asymmetry = 0.5, polarisation = 0.;
    /* several views: views[0] repeats the members above, views[k] is read
     * from the keys with " k" appended */
    struct View {
      double theta = 0., phi = 0.;
      bool have_anchor[2] = {false, false}, have_sides[2] = {false, false};
      double anchor[2] = {0., 0.}, sides[2] = {0., 0.};
    };
    long long nviews = 1;
    std::vector<View> views;

    void read_views(ParameterFile &params) {
      static const char *axis[2] = {"x", "y"};
      if (params.has_value("EmissionImages:number of views"))
        nviews = params.get_integer("EmissionImages:number of views", 1);
      if (nviews < 1 || nviews > CMI_GPU_MAX_VIEWS)
        throw ParameterError("EmissionImages:number of views must be 1.." +
                             std::to_string(CMI_GPU_MAX_VIEWS));
      views.assign(1, View());
      views[0].theta = theta;
      views[0].phi = phi;
      for (int a = 0; a < 2; ++a) {
        views[0].have_anchor[a] = have_anchor[a];
        views[0].have_sides[a] = have_sides[a];
        views[0].anchor[a] = anchor[a];
        views[0].sides[a] = sides[a];
      }
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
        for (int a = 0; a < 2; ++a) {
          const std::string ka =
              std::string("EmissionImages:anchor ") + axis[a] + n;
          const std::string ks =
              std::string("EmissionImages:sides ") + axis[a] + n;
          if (params.has_value(ka)) {
            v.have_anchor[a] = true;
            v.anchor[a] = params.get_physical_value(QUANTITY_LENGTH, ka, "0. m");
          }
          if (params.has_value(ks)) {
            v.have_sides[a] = true;
            v.sides[a] = params.get_physical_value(QUANTITY_LENGTH, ks, "1. m");
          }
          if (v.have_sides[a] && !(v.sides[a] > 0.))
            throw ParameterError("EmissionImages: the image sides must be "
                                 "positive");
        }
        views.push_back(v);
      }
    }

    void read(ParameterFile &params) {
      theta = params.get_physical_value(QUANTITY_ANGLE,
                                        "EmissionImages:view theta", "0. degrees");
      phi = params.get_physical_value(QUANTITY_ANGLE,
                                      "EmissionImages:view phi", "0. degrees");
      nx = params.get_integer("EmissionImages:image width", 200);
      ny = params.get_integer("EmissionImages:image height", 200);
      static const char *axis[2] = {"x", "y"};
      for (int a = 0; a < 2; ++a) {
        const std::string ka = std::string("EmissionImages:anchor ") + axis[a];
        const std::string ks = std::string("EmissionImages:sides ") + axis[a];
        if ((have_anchor[a] = params.has_value(ka)))
          anchor[a] = params.get_physical_value(QUANTITY_LENGTH, ka, "0. m");
        if ((have_sides[a] = params.has_value(ks)))
          sides[a] = params.get_physical_value(QUANTITY_LENGTH, ks, "1. m");
      }
      supersample = params.get_integer("EmissionImages:supersampling", 1);
      dust_cross_section = params.get_physical_value(
          QUANTITY_SURFACE_AREA,
          "EmissionImages:dust cross section per hydrogen", "0. m^2");
      type = params.get_string("EmissionImages:type", "BinaryArray");
      prefix = params.get_string("EmissionImages:filename prefix",
                                 "line_image");
      folder = params.get_string("EmissionImages:output folder", ".");
      if (!is_image_type(type))
        throw ParameterError("Unknown EmissionImages:type \"" + type +
                             "\" (BinaryArray or PGM)");
      if (nx <= 0 || ny <= 0 || nx * ny > (1ll << 28))
        throw ParameterError("EmissionImages: image width and height must be "
                             "positive, 2^28 pixels at most (" +
                             std::to_string(nx) + " x " + std::to_string(ny) +
                             " asked for)");
      if (supersample < 1 || supersample > 8)
        throw ParameterError("EmissionImages:supersampling must be 1..8");
      if (!(dust_cross_section >= 0.))
        throw ParameterError("EmissionImages:dust cross section per hydrogen "
                             "must not be negative");
      for (int a = 0; a < 2; ++a)
        if (have_sides[a] && !(sides[a] > 0.))
          throw ParameterError("EmissionImages: the image sides must be "
                               "positive");
      read_views(params);
      read_cubes(params, "EmissionImages", type);
      read_continuum(params, "EmissionImages", type);
      read_hi(params, "EmissionImages", type);
      /* (a key that is read shows in the used-values: with the switch
       * absent or off none of these is, the switch included) */
      /* (looked at like the switch above: a file without it, or with it
       * false, has the used-values it had) */
      if (params.peek_bool("EmissionImages:scattered cubes")) {
        if (!params.peek_bool("EmissionImages:scattering"))
          throw ParameterError("EmissionImages:scattered cubes needs "
                               "scattering: true");
        if (!cubes)
          throw ParameterError("EmissionImages:scattered cubes needs "
                               "velocity channels");
        scattered_cubes =
            params.get_bool("EmissionImages:scattered cubes", false);
      }
      /* (looked at like the switches above) */
      if (params.peek_bool("EmissionImages:Lyman alpha")) {
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
      if (!lyman_alpha && !params.peek_bool("EmissionImages:scattering"))
        return;
      if (params.peek_bool("EmissionImages:scattering"))
        scattering = params.get_bool("EmissionImages:scattering", false);
      npackets = params.get_integer("EmissionImages:number of packets",
                                    1000000);
      seed = params.get_integer("EmissionImages:random seed", 42);
      if (npackets <= 0)
        throw ParameterError("EmissionImages:number of packets must be "
                             "positive");
      if (seed < 0 || seed > 0xffffffffll)
        throw ParameterError("EmissionImages:random seed must fit 32 bits");
      static const char *keys[3] = {
          "EmissionImages:dust albedo", "EmissionImages:dust asymmetry",
          "EmissionImages:dust peak linear polarisation"};
      double *values[3] = {&albedo, &asymmetry, &polarisation};
      for (int k = 0; k < 3; ++k) {
        if (params.has_value(keys[k]))
          *values[k] = params.get_double(keys[k], *values[k]);
        else if (dust_cross_section > 0.)
          throw ParameterError(std::string(keys[k]) +
                               " is required for scattering off dust with a "
                               "cross section above 0");
      }
      if (!(albedo >= 0. && albedo <= 1.))
        throw ParameterError("EmissionImages:dust albedo must be in [0, 1]");
      if (!(asymmetry != 0. && std::fabs(asymmetry) < 1.))
        throw ParameterError("EmissionImages:dust asymmetry must be non-zero "
                             "and inside (-1, 1)");
    }
  };

  /* the EmissionSkyMaps: block (read only if the file has one) */
  struct SkyMapSettings : CubeSettings {
    std::array<double, 3> observer = {0., 0., 0.};
    long long nlon = 360, nlat = 180;
    std::array<double, 2> lon = {0., 0.}, lat = {0., 0.};
    double frame[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
    double dust_cross_section = 0.;
    std::string type, prefix, folder;
    /* scattered light (the keys below are read only if scattering is set) */
    bool scattering = false, direct_light = true;
    bool scattered_cubes = false; /* as ImageSettings' */
    long long npackets = 1000000, seed = 42;
    double albedo = 0., asymmetry = 0.5, polarisation = 0.;
    double exclusion_radius = 0.;
    double camera_lon_max = 0.; /* min(lon[1], lon[0] + 2 pi) */
    /* several observers: observers[0] repeats the members above,
     * observers[k] is read from the keys with " k" appended */
    struct Observer {
      std::array<double, 3> position = {0., 0., 0.};
      double frame[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
      double exclusion_radius = 0.;
      std::array<double, 3> velocity = {0., 0., 0.}; /* sky cubes */
    };
    long long nobservers = 1;
    std::vector<Observer> observers;

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

    /* the observers' positions and frames (the exclusion radii are read with
     * the scattering keys) */
    void read_observers(ParameterFile &params,
                        const std::array<double, 3> &pole,
                        const std::array<double, 3> &zero) {
      if (params.has_value("EmissionSkyMaps:number of observers"))
        nobservers =
            params.get_integer("EmissionSkyMaps:number of observers", 1);
      if (nobservers < 1 || nobservers > CMI_GPU_MAX_VIEWS)
        throw ParameterError("EmissionSkyMaps:number of observers must be "
                             "1.." + std::to_string(CMI_GPU_MAX_VIEWS));
      observers.assign(1, Observer());
      observers[0].position = observer;
      std::copy(frame, frame + 9, observers[0].frame);
      for (long long k = 1; k < nobservers; ++k) {
        const std::string n = " " + std::to_string(k);
        Observer o;
        const std::string key = "EmissionSkyMaps:observer position" + n;
        if (!params.has_value(key))
          throw ParameterError(key + " is required");
        o.position = params.get_physical_vector(QUANTITY_LENGTH, key, "");
        for (int a = 0; a < 3; ++a)
          if (!std::isfinite(o.position[a]))
            throw ParameterError(key + " must be finite");
        const std::string kpole = "EmissionSkyMaps:frame pole" + n;
        const std::string kzero = "EmissionSkyMaps:frame zero longitude" + n;
        const std::array<double, 3> p =
            params.has_value(kpole) ? params.get_double_vector(kpole, pole)
                                    : pole;
        const std::array<double, 3> z =
            params.has_value(kzero) ? params.get_double_vector(kzero, zero)
                                    : zero;
        make_frame(p, z, n, o.frame);
        observers.push_back(o);
      }
    }

    /* sky cubes: "observer velocity", and "observer velocity k" for observer
     * k >= 1 (observer 0's where the key is absent) */
    void read_observer_velocities(ParameterFile &params) {
      for (long long k = 0; k < nobservers; ++k) {
        const std::string key = "EmissionSkyMaps:observer velocity" +
                                (k ? " " + std::to_string(k) : std::string());
        Observer &o = observers[(size_t)k];
        if (k == 0 || params.has_value(key))
          o.velocity = params.get_physical_vector(
              QUANTITY_VELOCITY, key, "[0. m s^-1, 0. m s^-1, 0. m s^-1]");
        else
          o.velocity = observers[0].velocity;
        for (int a = 0; a < 3; ++a)
          if (!std::isfinite(o.velocity[a]))
            throw ParameterError(key + " must be finite");
      }
    }

    void read(ParameterFile &params) {
      if (!params.has_value("EmissionSkyMaps:observer position"))
        throw ParameterError("EmissionSkyMaps:observer position is required");
      observer = params.get_physical_vector(
          QUANTITY_LENGTH, "EmissionSkyMaps:observer position", "");
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
      dust_cross_section = params.get_physical_value(
          QUANTITY_SURFACE_AREA,
          "EmissionSkyMaps:dust cross section per hydrogen", "0. m^2");
      type = params.get_string("EmissionSkyMaps:type", "BinaryArray");
      prefix = params.get_string("EmissionSkyMaps:filename prefix", "sky_map");
      folder = params.get_string("EmissionSkyMaps:output folder", ".");
      if (!is_image_type(type))
        throw ParameterError("Unknown EmissionSkyMaps:type \"" + type +
                             "\" (BinaryArray or PGM)");
      for (int a = 0; a < 3; ++a)
        if (!std::isfinite(observer[a]))
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
      if (!(dust_cross_section >= 0.))
        throw ParameterError("EmissionSkyMaps:dust cross section per hydrogen "
                             "must not be negative");
      make_frame(pole, zero, "", frame);
      read_observers(params, pole, zero);
      read_cubes(params, "EmissionSkyMaps", type);
      if (cubes)
        read_observer_velocities(params);
      read_continuum(params, "EmissionSkyMaps", type);
      read_hi(params, "EmissionSkyMaps", type);
      /* (a key that is read shows in the used-values: with the switch
       * absent or off none of these is, the switch included) */
      /* (looked at like the switch above: a file without it, or with it
       * false, has the used-values it had) */
      if (params.peek_bool("EmissionSkyMaps:scattered cubes")) {
        if (!params.peek_bool("EmissionSkyMaps:scattering"))
          throw ParameterError("EmissionSkyMaps:scattered cubes needs "
                               "scattering: true");
        if (!cubes)
          throw ParameterError("EmissionSkyMaps:scattered cubes needs "
                               "velocity channels");
        scattered_cubes =
            params.get_bool("EmissionSkyMaps:scattered cubes", false);
      }
      if (params.peek_bool("EmissionSkyMaps:Lyman alpha"))
        throw ParameterError("EmissionSkyMaps:Lyman alpha is not supported: "
                             "the Lyman-alpha transfer serves the parallel "
                             "cameras of EmissionImages only");
      if (!params.peek_bool("EmissionSkyMaps:scattering"))
        return;
      scattering = params.get_bool("EmissionSkyMaps:scattering", false);
      npackets = params.get_integer("EmissionSkyMaps:number of packets",
                                    1000000);
      seed = params.get_integer("EmissionSkyMaps:random seed", 42);
      if (npackets <= 0)
        throw ParameterError("EmissionSkyMaps:number of packets must be "
                             "positive");
      if (seed < 0 || seed > 0xffffffffll)
        throw ParameterError("EmissionSkyMaps:random seed must fit 32 bits");
      static const char *keys[3] = {
          "EmissionSkyMaps:dust albedo", "EmissionSkyMaps:dust asymmetry",
          "EmissionSkyMaps:dust peak linear polarisation"};
      double *values[3] = {&albedo, &asymmetry, &polarisation};
      for (int k = 0; k < 3; ++k) {
        if (params.has_value(keys[k]))
          *values[k] = params.get_double(keys[k], *values[k]);
        else if (dust_cross_section > 0.)
          throw ParameterError(std::string(keys[k]) +
                               " is required for scattering off dust with a "
                               "cross section above 0");
      }
      if (!(albedo >= 0. && albedo <= 1.))
        throw ParameterError("EmissionSkyMaps:dust albedo must be in [0, 1]");
      if (!(asymmetry != 0. && std::fabs(asymmetry) < 1.))
        throw ParameterError("EmissionSkyMaps:dust asymmetry must be non-zero "
                             "and inside (-1, 1)");
      if (!params.has_value("EmissionSkyMaps:exclusion radius"))
        throw ParameterError("EmissionSkyMaps:exclusion radius is required "
                             "for scattering");
      exclusion_radius = params.get_physical_value(
          QUANTITY_LENGTH, "EmissionSkyMaps:exclusion radius", "0. m");
      if (!(exclusion_radius >= 0.) || !std::isfinite(exclusion_radius))
        throw ParameterError("EmissionSkyMaps:exclusion radius must be "
                             "finite and not negative");
      observers[0].exclusion_radius = exclusion_radius;
      for (long long k = 1; k < nobservers; ++k) {
        const std::string key =
            "EmissionSkyMaps:exclusion radius " + std::to_string(k);
        double r = exclusion_radius;
        if (params.has_value(key))
          r = params.get_physical_value(QUANTITY_LENGTH, key, "0. m");
        if (!(r >= 0.) || !std::isfinite(r))
          throw ParameterError(key + " must be finite and not negative");
        observers[(size_t)k].exclusion_radius = r;
      }
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
  static const AbsorptionLine *absorption_line(const std::string &name) {
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

public:
  /* EmissivityCalculationSimulation::do_simulation, :58-299 */
  static int do_simulation(const std::string &parameterfile_name,
                           const std::string &input_file_name, int device,
                           bool write_output, bool verbose,
                           bool describe = false) {
    auto status = [verbose](const std::string &text) {
      if (verbose)
        std::cout << text << std::endl;
    };
    ParameterFile params(parameterfile_name);
    std::vector<int32_t> lines;
    for (int32_t i = 0; i < CMI_GPU_NUMBER_OF_EMISSIONLINES; ++i)
      if (params.get_bool(
              std::string("EmissivityValues:") +
                  GpuIonizationSimulation::emission_line_name(i),
              false))
        lines.push_back(i);
    const bool do_images = params.has_block("EmissionImages");
    ImageSettings img;
    if (do_images)
      img.read(params);
    const bool do_sky = params.has_block("EmissionSkyMaps");
    SkyMapSettings sky;
    if (do_sky)
      sky.read(params);
    const bool do_absorption = params.has_block("AbsorptionSpectra");
    AbsorptionSettings absorption;
    if (do_absorption)
      absorption.read(params);
    if (describe && do_absorption) {
      absorption.describe(std::cout);
      /* a dry run that describes ends here: it needs no snapshot */
      if (!write_output)
        return 0;
    }
    if (write_output) {
      std::ofstream pfile(parameterfile_name + ".used-values");
      params.print_contents(pfile);
    }
    if (input_file_name.empty())
      throw ParameterError("No input file name provided (--file)!");
    status("Reading file \"" + input_file_name + "\"...");

    Hdf5Reader file(input_file_name);
    /* :101-117 */
    ParameterFile simulation_parameters;
    for (const auto &kv : file.open("/Parameters").attributes)
      simulation_parameters.add_value(kv.first,
                                      Hdf5Reader::as_string(kv.second));
    /* :123-147 */
    double unit_number_density_in_SI = 1., unit_temperature_in_SI = 1.;
    double unit_length_in_SI = 1.;
    if (file.exists("/Units")) {
      const Hdf5Reader::Object units = file.open("/Units");
      unit_length_in_SI =
          0.01 * Hdf5Reader::as_doubles(
                     units.attributes.at("Unit length in cgs (U_L)"))
                     .at(0);
      unit_number_density_in_SI =
          1. / unit_length_in_SI / unit_length_in_SI / unit_length_in_SI;
      unit_temperature_in_SI =
          Hdf5Reader::as_doubles(
              units.attributes.at("Unit temperature in cgs (U_T)"))
              .at(0);
    }
    /* :153-165: old parameter files name the abundances directly */
    double abundances[6];
    if (simulation_parameters.has_value("Abundances:helium")) {
      static const char *names[6] = {"helium", "carbon",  "nitrogen",
                                     "oxygen", "neon",    "sulphur"};
      static const double defaults[6] = {0.1,    2.2e-4, 4.e-5,
                                         3.3e-4, 5.e-5,  9.e-6};
      for (int i = 0; i < 6; ++i)
        abundances[i] = simulation_parameters.get_double(
            std::string("Abundances:") + names[i], defaults[i]);
    } else {
      const Abundances model(simulation_parameters);
      for (int i = 0; i < 6; ++i)
        abundances[i] = model.value[i];
    }

    /* :209-229 */
    std::vector<double> number_density =
        file.read_doubles("/PartType0/NumberDensity");
    std::vector<double> temperature =
        file.read_doubles("/PartType0/Temperature");
    const size_t size = number_density.size();
    if (temperature.size() != size)
      throw ParameterError("snapshot with " + std::to_string(size) +
                           " densities and " +
                           std::to_string(temperature.size()) +
                           " temperatures");
    const std::array<long long, 3> ncell =
        simulation_parameters.get_integer_vector("DensityGrid:number of cells",
                                                 {-1, -1, -1});
    if ((long long)size != ncell[0] * ncell[1] * ncell[2])
      throw ParameterError(
          "the snapshot does not hold DensityGrid:number of cells cells");
    std::vector<double> fractions((size_t)NUMBER_OF_IONNAMES * size);
    for (int ion = 0; ion < NUMBER_OF_IONNAMES; ++ion) {
      const std::string name =
          std::string("/PartType0/NeutralFraction") + ion_name(ion);
      if (!file.exists(name))
        throw ParameterError(std::string("Missing ionic fractions for \"") +
                             ion_name(ion) + "\"!");
      const std::vector<double> x = file.read_doubles(name);
      if (x.size() != size)
        throw ParameterError("dataset " + name + " has the wrong size");
      std::copy(x.begin(), x.end(), fractions.begin() + (size_t)ion * size);
    }
    for (size_t i = 0; i < size; ++i) {
      number_density[i] *= unit_number_density_in_SI;
      temperature[i] *= unit_temperature_in_SI;
    }

    /* images: the real grid. cell_of_row[i] = the cell row i of the file
     * describes (its midpoint, with the box anchor as the origin) */
    std::array<double, 3> box_anchor = {0., 0., 0.}, box_sides = {1., 1., 1.};
    std::vector<size_t> cell_of_row;
    if (((do_images || do_sky) && !lines.empty()) || do_absorption) {
      box_anchor = simulation_parameters.get_physical_vector(
          QUANTITY_LENGTH, "SimulationBox:anchor", "");
      box_sides = simulation_parameters.get_physical_vector(
          QUANTITY_LENGTH, "SimulationBox:sides", "");
      const std::vector<double> midpoints =
          file.read_doubles("/PartType0/Coordinates");
      if (midpoints.size() != 3 * size)
        throw ParameterError("snapshot with " + std::to_string(size) +
                             " cells and " +
                             std::to_string(midpoints.size() / 3) +
                             " coordinates");
      cell_of_row.resize(size);
      std::vector<char> seen(size, 0);
      for (size_t i = 0; i < size; ++i) {
        size_t index = 0;
        for (int a = 0; a < 3; ++a) {
          const double p = midpoints[3 * i + a] * unit_length_in_SI;
          const long long k = (long long)std::floor(ncell[a] * p / box_sides[a]);
          if (k < 0 || k >= ncell[a])
            throw ParameterError("EmissionImages: row " + std::to_string(i) +
                                 " of /PartType0/Coordinates lies outside "
                                 "the snapshot's box");
          index = index * (size_t)ncell[a] + (size_t)k;
        }
        if (seen[index])
          throw ParameterError(
              "EmissionImages: the snapshot's coordinates put two rows into "
              "cell " + std::to_string(index) + ": they are not one per cell "
              "of the grid");
        seen[index] = 1;
        cell_of_row[i] = index;
      }
    }

    /* cubes: the cells' velocities in the engine's cell order, [3][size] */
    auto cell_velocities = [&](const CubeSettings &cs,
                               const std::string &block) {
      std::vector<double> velocities;
      if (!cs.cubes || cell_of_row.empty() || cs.velocity_field == "Static")
        return velocities;
      velocities.assign(3 * size, 0.);
      if (cs.velocity_field == "Snapshot") {
        if (!file.exists("/PartType0/Velocities"))
          throw ParameterError(block + ":velocity field type Snapshot: "
                               "the snapshot has no dataset "
                               "/PartType0/Velocities");
        const std::vector<double> rows =
            file.read_doubles("/PartType0/Velocities");
        if (rows.size() != 3 * size)
          throw ParameterError("dataset /PartType0/Velocities has the wrong "
                               "size");
        double unit_time_in_SI = 1.;
        if (file.exists("/Units")) {
          const Hdf5Reader::Object units = file.open("/Units");
          const auto it = units.attributes.find("Unit time in cgs (U_t)");
          if (it != units.attributes.end())
            unit_time_in_SI = Hdf5Reader::as_doubles(it->second).at(0);
        }
        const double unit = unit_length_in_SI / unit_time_in_SI;
        for (size_t i = 0; i < size; ++i)
          for (int a = 0; a < 3; ++a)
            velocities[(size_t)a * size + cell_of_row[i]] =
                rows[3 * i + a] * unit;
      } else {
        size_t c = 0;
        for (long long i = 0; i < ncell[0]; ++i)
          for (long long j = 0; j < ncell[1]; ++j)
            for (long long k = 0; k < ncell[2]; ++k, ++c) {
              const long long idx[3] = {i, j, k};
              std::array<double, 3> r;
              for (int a = 0; a < 3; ++a)
                r[a] = box_anchor[a] +
                       (idx[a] + 0.5) * (box_sides[a] / ncell[a]);
              const std::array<double, 3> v = cs.velocity_at(r);
              for (int a = 0; a < 3; ++a)
                velocities[(size_t)a * size + c] = v[a];
            }
      }
      return velocities;
    };
    const std::vector<double> velocities =
        do_images ? cell_velocities(img, "EmissionImages")
                  : std::vector<double>();
    const std::vector<double> sky_velocities =
        do_sky ? cell_velocities(sky, "EmissionSkyMaps")
               : std::vector<double>();
    const std::vector<double> absorption_velocities =
        do_absorption ? cell_velocities(absorption, "AbsorptionSpectra")
                      : std::vector<double>();

    status("Starting emissivity calculation...");
    std::vector<double> values(lines.size() * size);
    if (!lines.empty() || do_absorption) {
      /* without images: the cells in the file's order on a device grid of
       * the same shape (every cell on its own: the shape only has to hold
       * them); with them, every cell in its place in the real box */
      const bool placed = !cell_of_row.empty();
      if (placed) {
        std::vector<double> n2(size), t2(size),
            f2((size_t)NUMBER_OF_IONNAMES * size);
        for (size_t i = 0; i < size; ++i) {
          const size_t c = cell_of_row[i];
          n2[c] = number_density[i];
          t2[c] = temperature[i];
          for (int ion = 0; ion < NUMBER_OF_IONNAMES; ++ion)
            f2[(size_t)ion * size + c] = fractions[(size_t)ion * size + i];
        }
        number_density.swap(n2);
        temperature.swap(t2);
        fractions.swap(f2);
      }
      cmi_gpu_config config = {};
      for (int a = 0; a < 3; ++a) {
        config.anchor[a] = placed ? box_anchor[a] : 0.;
        config.sides[a] = placed ? box_sides[a] : 1.;
        config.ncell[a] = (int32_t)ncell[a];
      }
      config.device = device;
      cmi_gpu_engine *engine = nullptr;
      check(cmi_gpu_create(&config, &engine), "cmi_gpu_create");
      int rc = cmi_gpu_set_abundances(engine, abundances);
      if (rc == CMI_GPU_OK)
        rc = cmi_gpu_upload_cells(engine, number_density.data(),
                                  temperature.data(), fractions.data());
      if (rc == CMI_GPU_OK && !lines.empty())
        rc = cmi_gpu_compute_emissivities(engine, (int32_t)lines.size(),
                                          lines.data(), 0, (int64_t)size,
                                          values.data());
      if (rc == CMI_GPU_OK && placed) {
        /* the datasets keep the file's order */
        std::vector<double> v2(values.size());
        for (size_t k = 0; k < lines.size(); ++k)
          for (size_t i = 0; i < size; ++i)
            v2[k * size + i] = values[k * size + cell_of_row[i]];
        values.swap(v2);
      }
      std::string written;
      /* "" for view 0, whose files keep their names */
      auto view_tag = [](size_t v) {
        return v ? "_view" + std::to_string(v) : std::string();
      };
      static const char *stokes[3] = {"_scattered_I", "_scattered_Q",
                                      "_scattered_U"};
      static const char *cube_stokes[3] = {
          "_scattered_cube_I", "_scattered_cube_Q", "_scattered_cube_U"};
      if (rc == CMI_GPU_OK && placed && do_images && !lines.empty()) {
        status("Rendering emission line images...");
        const size_t nviews = img.views.size();
        /* per view, default image: the rectangle around the box's projected
         * corners */
        std::vector<double> theta(nviews), phi(nviews), anchors(2 * nviews),
            sides(2 * nviews);
        for (size_t v = 0; v < nviews; ++v) {
          const ImageSettings::View &view = img.views[v];
          theta[v] = view.theta;
          phi[v] = view.phi;
          const double st = std::sin(view.theta), ct = std::cos(view.theta),
                       sp = std::sin(view.phi), cp = std::cos(view.phi);
          const double ex[3] = {-sp, cp, 0.};
          const double ey[3] = {-ct * cp, -ct * sp, st};
          double lo[2] = {HUGE_VAL, HUGE_VAL}, hi[2] = {-HUGE_VAL, -HUGE_VAL};
          for (int corner = 0; corner < 8; ++corner) {
            double p[2] = {0., 0.};
            for (int a = 0; a < 3; ++a) {
              const double x =
                  box_anchor[a] + ((corner >> a) & 1) * box_sides[a];
              p[0] += x * ex[a];
              p[1] += x * ey[a];
            }
            for (int k = 0; k < 2; ++k) {
              lo[k] = std::min(lo[k], p[k]);
              hi[k] = std::max(hi[k], p[k]);
            }
          }
          for (int k = 0; k < 2; ++k) {
            anchors[2 * v + k] = view.have_anchor[k] ? view.anchor[k] : lo[k];
            sides[2 * v + k] =
                view.have_sides[k] ? view.sides[k] : hi[k] - anchors[2 * v + k];
          }
        }
        const size_t npixel = (size_t)img.nx * (size_t)img.ny;
        std::vector<double> images(lines.size() * npixel);
        /* cubes: of the flagged entries that are the line of one ion */
        std::vector<int32_t> cube_lines;
        std::vector<double> cube;
        if (img.cubes) {
          for (const int32_t line : lines)
            if (cmi_gpu_emission_line_atomic_weight(line) > 0.)
              cube_lines.push_back(line);
            else
              std::cerr << "EmissionImages: "
                        << GpuIonizationSimulation::emission_line_name(line)
                        << " is not the line of one ion: no cube, the image "
                           "alone" << std::endl;
          if ((double)cube_lines.size() * (double)img.nchan * (double)npixel >
              (double)(1ll << 28))
            throw ParameterError(
                "EmissionImages: " + std::to_string(cube_lines.size()) +
                " cubes of " + std::to_string(img.nchan) + " channels of " +
                std::to_string(img.nx) + " x " + std::to_string(img.ny) +
                " pixels: more than 2^28 values in one call");
          cube.resize(cube_lines.size() * (size_t)img.nchan * npixel);
          if ((!cube_lines.empty() || img.hi_cube) && !velocities.empty())
            rc = cmi_gpu_set_cell_velocities(engine, velocities.data());
        }
        for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
          rc = cmi_gpu_render_line_images(
              engine, (int32_t)lines.size(), lines.data(), theta[v], phi[v],
              (int32_t)img.nx, (int32_t)img.ny, anchors.data() + 2 * v,
              sides.data() + 2 * v, (int32_t)img.supersample,
              img.dust_cross_section, images.data());
          if (rc == CMI_GPU_OK && write_output)
            for (size_t k = 0; k < lines.size(); ++k)
              written += " " + write_image(
                  img.folder + "/" + img.prefix + "_" +
                      GpuIonizationSimulation::emission_line_name(lines[k]) +
                      view_tag(v),
                  img.type, images.data() + k * npixel, img.nx, img.ny, 1.);
          if (rc == CMI_GPU_OK && !cube_lines.empty()) {
            rc = cmi_gpu_render_line_cube(
                engine, (int32_t)cube_lines.size(), cube_lines.data(),
                theta[v], phi[v], (int32_t)img.nx, (int32_t)img.ny,
                anchors.data() + 2 * v, sides.data() + 2 * v,
                (int32_t)img.supersample, img.dust_cross_section,
                (int32_t)img.nchan, img.vmin, img.vmax, img.sigma_turb,
                cube.data());
            if (rc == CMI_GPU_OK && write_output)
              for (size_t k = 0; k < cube_lines.size(); ++k)
                written += " " + write_cube(
                    img.folder + "/" + img.prefix + "_" +
                        GpuIonizationSimulation::emission_line_name(
                            cube_lines[k]) +
                        "_cube" + view_tag(v),
                    cube.data() + k * (size_t)img.nchan * npixel, img.nchan,
                    img.nx, img.ny);
          }
        }
        if (rc == CMI_GPU_OK && img.continuum) {
          status("Rendering radio continuum images...");
          const size_t nf = img.continuum_frequencies.size();
          if ((double)nf * (double)npixel > (double)(1ll << 28))
            throw ParameterError(
                "EmissionImages: " + std::to_string(nf) +
                " continuum frequencies of " + std::to_string(img.nx) +
                " x " + std::to_string(img.ny) +
                " pixels: more than 2^28 values in one call");
          std::vector<double> continuum(nf * npixel);
          for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
            rc = cmi_gpu_render_continuum_images(
                engine, (int32_t)nf, img.continuum_frequencies.data(),
                img.continuum_background.data(), theta[v], phi[v],
                (int32_t)img.nx, (int32_t)img.ny, anchors.data() + 2 * v,
                sides.data() + 2 * v, (int32_t)img.supersample,
                continuum.data());
            if (rc == CMI_GPU_OK && write_output)
              written += " " + write_cube(img.folder + "/" + img.prefix +
                                              "_continuum" + view_tag(v),
                                          continuum.data(), (long long)nf,
                                          img.nx, img.ny);
          }
          if (rc == CMI_GPU_OK && write_output)
            written += " " + img.write_continuum_frequencies(
                                 img.folder + "/" + img.prefix +
                                 "_continuum_frequencies");
        }
        /* with "HI Lyman alpha coupling" the Lyman-alpha run comes first and
         * leaves the spin temperature of the cells here */
        std::vector<double> coupled_spin;
        const auto shoot_lyman_alpha = [&]() {
          if (!(rc == CMI_GPU_OK && img.lyman_alpha))
            return;
          status("Shooting the Lyman alpha packets through the H I...");
          /* the source: the cells' recombinations; the scatterers: the
           * cells' own H I at their temperatures, and the block's dust */
          std::vector<double> source(size);
          rc = cmi_gpu_lyman_alpha_emissivity(engine, source.data());
          if (rc == CMI_GPU_OK)
            rc = cmi_gpu_set_dust_scattering_per_hydrogen(
                engine, img.asymmetry, img.polarisation, img.albedo,
                img.dust_cross_section);
          if (rc == CMI_GPU_OK)
            rc = nviews == 1
                     ? cmi_gpu_set_ccd_image(engine, theta[0], phi[0],
                                             (int32_t)img.nx, (int32_t)img.ny,
                                             anchors.data(), sides.data())
                     : cmi_gpu_set_ccd_images(
                           engine, (int32_t)nviews, theta.data(), phi.data(),
                           (int32_t)img.nx, (int32_t)img.ny, anchors.data(),
                           sides.data());
          if (rc == CMI_GPU_OK && !velocities.empty())
            rc = cmi_gpu_set_cell_velocities(engine, velocities.data());
          if (rc == CMI_GPU_OK)
            rc = cmi_gpu_set_cell_source_field(engine, source.data());
          if (rc == CMI_GPU_OK)
            rc = cmi_gpu_set_lyman_alpha(
                engine, (int32_t)img.nchan, img.vmin, img.vmax, img.sigma_turb,
                img.lya_core_skip, (uint64_t)img.lya_max_scatter, nullptr,
                nullptr);
          if (rc == CMI_GPU_OK && img.lya_field)
            rc = cmi_gpu_set_lya_field(engine, 1);
          if (rc == CMI_GPU_OK)
            rc = cmi_gpu_lya_shoot(engine, (uint32_t)img.seed, 0,
                                   (uint64_t)img.npackets);
          double total = 0.;
          if (rc == CMI_GPU_OK)
            rc = cmi_gpu_get_cell_source(engine, &total, nullptr, nullptr);
          const size_t nvalue = (size_t)img.nchan * npixel;
          std::vector<double> lya_image(npixel), lya_cube(nvalue);
          for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
            rc = cmi_gpu_download_lya_view(engine, (int32_t)v,
                                           lya_image.data(), lya_cube.data());
            const double pixel_area = sides[2 * v] * sides[2 * v + 1] /
                                      ((double)img.nx * (double)img.ny);
            const double scale = total / ((double)img.npackets * pixel_area);
            for (double &value : lya_cube)
              value *= scale;
            if (rc == CMI_GPU_OK && write_output) {
              written += " " + write_image(img.folder + "/" + img.prefix +
                                               "_LymanAlpha_image" +
                                               view_tag(v),
                                           img.type, lya_image.data(), img.nx,
                                           img.ny, scale);
              written += " " + write_cube(img.folder + "/" + img.prefix +
                                              "_LymanAlpha_cube" + view_tag(v),
                                          lya_cube.data(), img.nchan, img.nx,
                                          img.ny);
            }
          }
          if (rc == CMI_GPU_OK && img.lya_field) {
            /* rows {L, S_H, S_d, G[3], N_H, N_d} -> [5][ncell] in physical
             * units; the rate per atom is the engine's (it knows the records'
             * n_HI), 0 if the core is skipped */
            const double per_packet = total / (double)img.npackets;
            const double volume = (box_sides[0] / ncell[0]) *
                                  (box_sides[1] / ncell[1]) *
                                  (box_sides[2] / ncell[2]);
            const double per_volume = per_packet / (299792458. * volume);
            std::vector<double> rows(8 * size), field(5 * size, 0.),
                spin(size);
            rc = cmi_gpu_download_lya_field(engine, rows.data());
            if (rc == CMI_GPU_OK && !(img.lya_core_skip > 0.))
              rc = cmi_gpu_lya_spin_temperature(
                  engine, per_packet,
                  img.lya_coupling ? img.hi_background_temperature : 1.,
                  img.lya_coupling ? 1 : 0, field.data() + size, spin.data());
            for (size_t c = 0; c < size; ++c) {
              field[c] = rows[8 * c] * per_volume;
              for (size_t a = 0; a < 3; ++a)
                field[(2 + a) * size + c] = rows[8 * c + 3 + a] * per_volume;
            }
            if (img.lya_coupling)
              coupled_spin = spin;
            if (rc == CMI_GPU_OK && write_output) {
              written += " " + write_cube(img.folder + "/" + img.prefix +
                                              "_LymanAlpha_field",
                                          field.data(), 5 * ncell[0], ncell[1],
                                          ncell[2]);
              if (img.lya_coupling)
                written += " " + write_cube(img.folder + "/" + img.prefix +
                                                "_HI_spin_temperature",
                                            spin.data(), ncell[0], ncell[1],
                                            ncell[2]);
            }
          }
          if (rc == CMI_GPU_OK)
            rc = cmi_gpu_set_lyman_alpha(engine, 0, 0., 1., 0., 0., 1, nullptr,
                                         nullptr);
        };
        const auto render_hi_cubes = [&]() {
          if (!(rc == CMI_GPU_OK && img.hi_cube))
            return;
          status("Rendering H I cubes...");
          if ((double)img.nchan * (double)npixel > (double)(1ll << 28))
            throw ParameterError(
                "EmissionImages: an H I cube of " + std::to_string(img.nchan) +
                " channels of " + std::to_string(img.nx) + " x " +
                std::to_string(img.ny) +
                " pixels: more than 2^28 values in one call");
          std::vector<double> hi((size_t)img.nchan * npixel);
          for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
            rc = cmi_gpu_render_hi_cube(
                engine, theta[v], phi[v], (int32_t)img.nx, (int32_t)img.ny,
                anchors.data() + 2 * v, sides.data() + 2 * v,
                (int32_t)img.supersample, (int32_t)img.nchan, img.vmin,
                img.vmax, img.sigma_turb,
                img.lya_coupling ? 2 : img.hi_spin_mode,
                img.lya_coupling ? coupled_spin.data()
                                 : &img.hi_spin_temperature,
                img.hi_free_free ? 1 : 0, img.hi_background_temperature,
                hi.data());
            if (rc == CMI_GPU_OK && write_output)
              written += " " + write_cube(img.folder + "/" + img.prefix +
                                              "_HI_cube" + view_tag(v),
                                          hi.data(), img.nchan, img.nx, img.ny);
          }
        };
        if (img.lya_coupling)
          shoot_lyman_alpha();
        render_hi_cubes();
        if (rc == CMI_GPU_OK && img.scattering) {
          status("Shooting the lines' packets through the dust...");
          rc = cmi_gpu_set_dust_scattering_per_hydrogen(
              engine, img.asymmetry, img.polarisation, img.albedo,
              img.dust_cross_section);
          /* one view: the single camera, as ever; several: one run fills
           * them all */
          if (rc == CMI_GPU_OK)
            rc = nviews == 1
                     ? cmi_gpu_set_ccd_image(engine, theta[0], phi[0],
                                             (int32_t)img.nx, (int32_t)img.ny,
                                             anchors.data(), sides.data())
                     : cmi_gpu_set_ccd_images(
                           engine, (int32_t)nviews, theta.data(), phi.data(),
                           (int32_t)img.nx, (int32_t)img.ny, anchors.data(),
                           sides.data());
          std::vector<double> iqu(3 * npixel);
          std::vector<double> scattered_cube(
              img.scattered_cubes ? 3 * (size_t)img.nchan * npixel : 0);
          for (size_t k = 0; rc == CMI_GPU_OK && k < lines.size(); ++k) {
            double total = 0.;
            rc = cmi_gpu_set_cell_source_line(engine, lines[k]);
            /* cube mode for the lines of one ion (it resets the image); the
             * velocities are those the ray-traced cubes were given */
            const bool with_cube =
                img.scattered_cubes &&
                cmi_gpu_emission_line_atomic_weight(lines[k]) > 0.;
            if (rc == CMI_GPU_OK && img.scattered_cubes)
              rc = cmi_gpu_set_scattered_cube(
                  engine, with_cube ? (int32_t)img.nchan : 0, img.vmin,
                  img.vmax, img.sigma_turb, nullptr, nullptr);
            if (rc == CMI_GPU_OK)
              rc = cmi_gpu_reset_image(engine);
            if (rc == CMI_GPU_OK)
              rc = cmi_gpu_dust_shoot(engine, (uint32_t)img.seed, 0,
                                      (uint64_t)img.npackets);
            if (rc == CMI_GPU_OK)
              rc = cmi_gpu_get_cell_source(engine, &total, nullptr, nullptr);
            for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
              rc = cmi_gpu_download_image_view(engine, (int32_t)v, iqu.data(),
                                               iqu.data() + npixel,
                                               iqu.data() + 2 * npixel);
              const double pixel_area = sides[2 * v] * sides[2 * v + 1] /
                                        ((double)img.nx * (double)img.ny);
              if (rc == CMI_GPU_OK && write_output)
                for (int j = 0; j < 3; ++j)
                  written += " " + write_image(
                      img.folder + "/" + img.prefix + "_" +
                          GpuIonizationSimulation::emission_line_name(
                              lines[k]) +
                          view_tag(v) + stokes[j],
                      img.type, iqu.data() + j * npixel, img.nx, img.ny,
                      total / ((double)img.npackets * pixel_area));
              if (rc == CMI_GPU_OK && with_cube) {
                const size_t nvalue = (size_t)img.nchan * npixel;
                rc = cmi_gpu_download_cube_view(
                    engine, (int32_t)v, scattered_cube.data(),
                    scattered_cube.data() + nvalue,
                    scattered_cube.data() + 2 * nvalue);
                const double scale =
                    total / ((double)img.npackets * pixel_area);
                for (double &value : scattered_cube)
                  value *= scale;
                if (rc == CMI_GPU_OK && write_output)
                  for (int j = 0; j < 3; ++j)
                    written += " " + write_cube(
                        img.folder + "/" + img.prefix + "_" +
                            GpuIonizationSimulation::emission_line_name(
                                lines[k]) +
                            view_tag(v) + cube_stokes[j],
                        scattered_cube.data() + j * nvalue, img.nchan, img.nx,
                        img.ny);
              }
            }
          }
          if (rc == CMI_GPU_OK && img.scattered_cubes)
            rc = cmi_gpu_set_scattered_cube(engine, 0, 0., 1., 0., nullptr,
                                            nullptr);
        }
        if (!img.lya_coupling)
          shoot_lyman_alpha();
      }
      if (rc == CMI_GPU_OK && placed && do_sky && !lines.empty()) {
        status("Rendering emission line sky maps...");
        const size_t nviews = sky.observers.size();
        const size_t npixel = (size_t)sky.nlon * (size_t)sky.nlat;
        std::vector<double> maps(lines.size() * npixel);
        /* cubes: of the flagged entries that are the line of one ion */
        std::vector<int32_t> cube_lines;
        std::vector<double> cube;
        if (sky.cubes) {
          for (const int32_t line : lines)
            if (cmi_gpu_emission_line_atomic_weight(line) > 0.)
              cube_lines.push_back(line);
            else
              std::cerr << "EmissionSkyMaps: "
                        << GpuIonizationSimulation::emission_line_name(line)
                        << " is not the line of one ion: no cube, the map "
                           "alone" << std::endl;
          if ((double)cube_lines.size() * (double)sky.nchan * (double)npixel >
              (double)(1ll << 28))
            throw ParameterError(
                "EmissionSkyMaps: " + std::to_string(cube_lines.size()) +
                " cubes of " + std::to_string(sky.nchan) + " channels of " +
                std::to_string(sky.nlon) + " x " + std::to_string(sky.nlat) +
                " pixels: more than 2^28 values in one call");
          cube.resize(cube_lines.size() * (size_t)sky.nchan * npixel);
          /* (the block's own field, whatever EmissionImages: left) */
          if (!cube_lines.empty() || sky.hi_cube)
            rc = cmi_gpu_set_cell_velocities(
                engine,
                sky_velocities.empty() ? nullptr : sky_velocities.data());
        }
        for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
          rc = cmi_gpu_render_line_sky_map(
              engine, (int32_t)lines.size(), lines.data(),
              sky.observers[v].position.data(), sky.observers[v].frame,
              sky.lon[0], sky.lon[1], sky.lat[0], sky.lat[1],
              (int32_t)sky.nlon, (int32_t)sky.nlat, sky.dust_cross_section,
              maps.data());
          if (rc == CMI_GPU_OK && write_output)
            for (size_t k = 0; k < lines.size(); ++k)
              written += " " + write_image(
                  sky.folder + "/" + sky.prefix + "_" +
                      GpuIonizationSimulation::emission_line_name(lines[k]) +
                      view_tag(v),
                  sky.type, maps.data() + k * npixel, sky.nlon, sky.nlat, 1.);
          if (rc == CMI_GPU_OK && !cube_lines.empty()) {
            rc = cmi_gpu_render_line_sky_map_cube(
                engine, (int32_t)cube_lines.size(), cube_lines.data(),
                sky.observers[v].position.data(), sky.observers[v].frame,
                sky.lon[0], sky.lon[1], sky.lat[0], sky.lat[1],
                (int32_t)sky.nlon, (int32_t)sky.nlat, sky.dust_cross_section,
                sky.observers[v].velocity.data(), (int32_t)sky.nchan, sky.vmin,
                sky.vmax, sky.sigma_turb, cube.data());
            if (rc == CMI_GPU_OK && write_output)
              for (size_t k = 0; k < cube_lines.size(); ++k)
                written += " " + write_cube(
                    sky.folder + "/" + sky.prefix + "_" +
                        GpuIonizationSimulation::emission_line_name(
                            cube_lines[k]) +
                        "_cube" + view_tag(v),
                    cube.data() + k * (size_t)sky.nchan * npixel, sky.nchan,
                    sky.nlon, sky.nlat);
          }
        }
        if (rc == CMI_GPU_OK && sky.continuum) {
          status("Rendering radio continuum sky maps...");
          const size_t nf = sky.continuum_frequencies.size();
          if ((double)nf * (double)npixel > (double)(1ll << 28))
            throw ParameterError(
                "EmissionSkyMaps: " + std::to_string(nf) +
                " continuum frequencies of " + std::to_string(sky.nlon) +
                " x " + std::to_string(sky.nlat) +
                " pixels: more than 2^28 values in one call");
          std::vector<double> continuum(nf * npixel);
          for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
            rc = cmi_gpu_render_continuum_sky_map(
                engine, (int32_t)nf, sky.continuum_frequencies.data(),
                sky.continuum_background.data(),
                sky.observers[v].position.data(), (int32_t)sky.nlon,
                (int32_t)sky.nlat, sky.lon.data(), sky.lat.data(),
                sky.observers[v].frame, continuum.data());
            if (rc == CMI_GPU_OK && write_output)
              written += " " + write_cube(sky.folder + "/" + sky.prefix +
                                              "_continuum" + view_tag(v),
                                          continuum.data(), (long long)nf,
                                          sky.nlon, sky.nlat);
          }
          if (rc == CMI_GPU_OK && write_output)
            written += " " + sky.write_continuum_frequencies(
                                 sky.folder + "/" + sky.prefix +
                                 "_continuum_frequencies");
        }
        if (rc == CMI_GPU_OK && sky.hi_cube) {
          status("Rendering H I sky cubes...");
          if ((double)sky.nchan * (double)npixel > (double)(1ll << 28))
            throw ParameterError(
                "EmissionSkyMaps: an H I cube of " +
                std::to_string(sky.nchan) + " channels of " +
                std::to_string(sky.nlon) + " x " + std::to_string(sky.nlat) +
                " pixels: more than 2^28 values in one call");
          std::vector<double> hi((size_t)sky.nchan * npixel);
          for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
            rc = cmi_gpu_render_hi_sky_map_cube(
                engine, sky.observers[v].position.data(),
                sky.observers[v].frame, sky.lon[0], sky.lon[1], sky.lat[0],
                sky.lat[1], (int32_t)sky.nlon, (int32_t)sky.nlat,
                sky.observers[v].velocity.data(), (int32_t)sky.nchan, sky.vmin,
                sky.vmax, sky.sigma_turb, sky.hi_spin_mode,
                &sky.hi_spin_temperature, sky.hi_free_free ? 1 : 0,
                sky.hi_background_temperature, hi.data());
            if (rc == CMI_GPU_OK && write_output)
              written += " " + write_cube(sky.folder + "/" + sky.prefix +
                                              "_HI_cube" + view_tag(v),
                                          hi.data(), sky.nchan, sky.nlon,
                                          sky.nlat);
          }
        }
        if (rc == CMI_GPU_OK && sky.scattering) {
          status("Shooting the lines' packets towards the observer...");
          std::vector<double> omega(nviews * npixel), iqu(3 * npixel);
          std::vector<double> origins(3 * nviews), frames(9 * nviews),
              radii(nviews);
          for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
            const SkyMapSettings::Observer &o = sky.observers[v];
            std::copy(o.position.begin(), o.position.end(),
                      origins.begin() + 3 * v);
            std::copy(o.frame, o.frame + 9, frames.begin() + 9 * v);
            radii[v] = o.exclusion_radius;
            rc = cmi_gpu_sky_map_directions(
                o.frame, sky.lon[0], sky.camera_lon_max, sky.lat[0],
                sky.lat[1], (int32_t)sky.nlon, (int32_t)sky.nlat, nullptr,
                omega.data() + v * npixel);
          }
          if (rc == CMI_GPU_OK)
            rc = cmi_gpu_set_dust_scattering_per_hydrogen(
                engine, sky.asymmetry, sky.polarisation, sky.albedo,
                sky.dust_cross_section);
          /* one observer: the single camera, as ever; several: one run fills
           * them all */
          if (rc == CMI_GPU_OK)
            rc = nviews == 1
                     ? cmi_gpu_set_sky_camera(
                           engine, origins.data(), frames.data(), sky.lon[0],
                           sky.camera_lon_max, sky.lat[0], sky.lat[1],
                           (int32_t)sky.nlon, (int32_t)sky.nlat, radii[0],
                           sky.direct_light ? 1 : 0)
                     : cmi_gpu_set_sky_cameras(
                           engine, (int32_t)nviews, origins.data(),
                           frames.data(), sky.lon[0], sky.camera_lon_max,
                           sky.lat[0], sky.lat[1], (int32_t)sky.nlon,
                           (int32_t)sky.nlat, radii.data(),
                           sky.direct_light ? 1 : 0);
          std::vector<double> scattered_cube(
              sky.scattered_cubes ? 3 * (size_t)sky.nchan * npixel : 0);
          std::vector<double> observer_velocities(3 * nviews);
          for (size_t v = 0; v < nviews; ++v)
            std::copy(sky.observers[v].velocity.begin(),
                      sky.observers[v].velocity.end(),
                      observer_velocities.begin() + 3 * v);
          for (size_t k = 0; rc == CMI_GPU_OK && k < lines.size(); ++k) {
            double total = 0.;
            rc = cmi_gpu_set_cell_source_line(engine, lines[k]);
            const bool with_cube =
                sky.scattered_cubes &&
                cmi_gpu_emission_line_atomic_weight(lines[k]) > 0.;
            if (rc == CMI_GPU_OK && sky.scattered_cubes)
              rc = cmi_gpu_set_scattered_cube(
                  engine, with_cube ? (int32_t)sky.nchan : 0, sky.vmin,
                  sky.vmax, sky.sigma_turb, nullptr,
                  observer_velocities.data());
            if (rc == CMI_GPU_OK)
              rc = cmi_gpu_reset_image(engine);
            if (rc == CMI_GPU_OK)
              rc = cmi_gpu_dust_shoot(engine, (uint32_t)sky.seed, 0,
                                      (uint64_t)sky.npackets);
            if (rc == CMI_GPU_OK)
              rc = cmi_gpu_get_cell_source(engine, &total, nullptr, nullptr);
            for (size_t v = 0; rc == CMI_GPU_OK && v < nviews; ++v) {
              rc = cmi_gpu_download_image_view(engine, (int32_t)v, iqu.data(),
                                               iqu.data() + npixel,
                                               iqu.data() + 2 * npixel);
              if (rc != CMI_GPU_OK)
                break;
              /* W m^-2 sr^-1: x L_total / packets / the pixel's solid angle,
               * in the order the Python call multiplies */
              const double per_packet = total / (double)sky.npackets;
              for (int j = 0; j < 3; ++j)
                for (size_t i = 0; i < npixel; ++i)
                  iqu[j * npixel + i] = iqu[j * npixel + i] * per_packet /
                                        omega[v * npixel + i];
              if (write_output)
                for (int j = 0; j < 3; ++j)
                  written += " " + write_image(
                      sky.folder + "/" + sky.prefix + "_" +
                          GpuIonizationSimulation::emission_line_name(
                              lines[k]) +
                          view_tag(v) + stokes[j],
                      sky.type, iqu.data() + j * npixel, sky.nlon, sky.nlat,
                      1.);
              if (with_cube) {
                const size_t nvalue = (size_t)sky.nchan * npixel;
                rc = cmi_gpu_download_cube_view(
                    engine, (int32_t)v, scattered_cube.data(),
                    scattered_cube.data() + nvalue,
                    scattered_cube.data() + 2 * nvalue);
                if (rc != CMI_GPU_OK)
                  break;
                for (size_t i = 0; i < 3 * nvalue; ++i)
                  scattered_cube[i] = scattered_cube[i] * per_packet /
                                      omega[v * npixel + i % npixel];
                if (write_output)
                  for (int j = 0; j < 3; ++j)
                    written += " " + write_cube(
                        sky.folder + "/" + sky.prefix + "_" +
                            GpuIonizationSimulation::emission_line_name(
                                lines[k]) +
                            view_tag(v) + cube_stokes[j],
                        scattered_cube.data() + j * nvalue, sky.nchan,
                        sky.nlon, sky.nlat);
              }
            }
          }
          if (rc == CMI_GPU_OK && sky.scattered_cubes)
            rc = cmi_gpu_set_scattered_cube(engine, 0, 0., 1., 0., nullptr,
                                            nullptr);
        }
      }
      if (rc == CMI_GPU_OK && do_absorption) {
        status("Rendering absorption spectra...");
        const AbsorptionSettings &ab = absorption;
        const size_t nrays = ab.lengths.size(), nl = ab.lines.size();
        std::vector<int32_t> ions(nl);
        std::vector<double> weights(nl), S(nl), g(nl);
        for (size_t l = 0; l < nl; ++l) {
          ions[l] = ab.lines[l]->ion;
          weights[l] = ab.lines[l]->weight;
          S[l] = ab.lines[l]->S();
          g[l] = ab.lines[l]->g();
        }
        std::vector<double> tau(nrays * nl * (size_t)ab.nchan), N(nrays * nl);
        /* the block's own velocity field, or none */
        rc = cmi_gpu_set_cell_velocities(
            engine, absorption_velocities.empty()
                        ? nullptr
                        : absorption_velocities.data());
        if (rc == CMI_GPU_OK)
          rc = cmi_gpu_render_absorption_spectra(
              engine, (int32_t)nl, ions.data(), weights.data(), S.data(),
              g.data(), ab.sigma_turb, (int64_t)nrays, ab.origins.data(),
              ab.directions.data(), ab.lengths.data(), ab.velocity.data(),
              (int32_t)ab.nchan, ab.vmin, ab.vmax, tau.data(), N.data());
        if (rc == CMI_GPU_OK && write_output) {
          const std::string base =
              ab.folder + "/" + ab.prefix + "_absorption_";
          written += " " + write_cube(base + "tau", tau.data(),
                                      (long long)nrays, (long long)nl,
                                      ab.nchan);
          const std::string filename = base + "columns.txt";
          std::FILE *out = std::fopen(filename.c_str(), "w");
          if (!out)
            throw std::runtime_error("Could not write " + filename);
          const double dv = (ab.vmax - ab.vmin) / (double)ab.nchan;
          for (size_t r = 0; r < nrays; ++r)
            for (size_t l = 0; l < nl; ++l) {
              /* W = (lambda0 / c) sum_c (1 - exp(-tau_c)) dv */
              double sum = 0.;
              const double *t = tau.data() + (r * nl + l) * (size_t)ab.nchan;
              for (long long c = 0; c < ab.nchan; ++c)
                sum += -std::expm1(-t[c]);
              std::fprintf(out, "%zu %s %.17g %.17g\n", r, ab.lines[l]->name,
                           N[r * nl + l],
                           (ab.lines[l]->wavelength / constants::lightspeed) *
                               sum * dv);
            }
          std::fclose(out);
          written += " " + filename;
        }
      }
      const std::string message = rc ? cmi_gpu_last_error() : "";
      cmi_gpu_destroy(engine);
      if (rc)
        throw std::runtime_error("emissivity calculation: " + message);
      if (!written.empty())
        status("Wrote" + written + ".");
    }
    status("Finished emissivity calculation.");

    /* :181-193,258-263: the lines as datasets of /PartType0 (existing ones
     * are overwritten). Everything else in the file is carried over. */
    Hdf5Writer out;
    std::vector<std::vector<double>> kept; /* alive until out.write() */
    const Hdf5Reader::Object root = file.open("/");
    size_t ndatasets = 0;
    for (const auto &g : root.members)
      ndatasets += file.object(g.second).members.size();
    kept.reserve(ndatasets);
    for (const auto &g : root.members) {
      const Hdf5Reader::Object group = file.object(g.second);
      if (!group.is_group)
        throw ParameterError("\"/" + g.first + "\" is not a group: this file "
                             "cannot be rewritten with the lines added");
      out.create_group(g.first);
      for (const auto &a : group.attributes)
        out.attribute_raw(g.first, a.first, a.second.type.cls,
                          a.second.type.size, a.second.type.is_signed,
                          a.second.dims, a.second.data);
      for (const auto &d : group.members) {
        bool replaced = false;
        if (g.first == "PartType0")
          for (int32_t line : lines)
            replaced = replaced ||
                       d.first ==
                           GpuIonizationSimulation::emission_line_name(line);
        if (replaced) {
          std::cout << "Warning: dataset \"" << d.first
                    << "\" already exists! Values will be overwritten!"
                    << std::endl;
          continue;
        }
        const Hdf5Reader::Object ds = file.object(d.second);
        if (ds.is_group || ds.type.cls != 1 || ds.type.size != 8)
          throw ParameterError("\"/" + g.first + "/" + d.first +
                               "\" is not a dataset of doubles: this file "
                               "cannot be rewritten with the lines added");
        const std::vector<uint8_t> raw = file.raw(ds);
        kept.emplace_back(raw.size() / 8);
        std::memcpy(kept.back().data(), raw.data(), raw.size());
        const std::vector<double> *v = &kept.back();
        out.dataset(g.first, d.first, ds.dims, [v](std::ostream &os) {
          os.write(reinterpret_cast<const char *>(v->data()), 8 * v->size());
        });
      }
    }
    for (size_t k = 0; k < lines.size(); ++k) {
      const double *v = values.data() + k * size;
      out.dataset("PartType0",
                  GpuIonizationSimulation::emission_line_name(lines[k]),
                  {size}, [v, size](std::ostream &os) {
                    os.write(reinterpret_cast<const char *>(v), 8 * size);
                  });
    }
    const std::string temporary = input_file_name + ".tmp";
    out.write(temporary);
    if (std::rename(temporary.c_str(), input_file_name.c_str()) != 0)
      throw std::runtime_error("could not replace \"" + input_file_name +
                               "\"");
    status("Closed file.");
    return 0;
  }
};

} // namespace cmi

#endif
