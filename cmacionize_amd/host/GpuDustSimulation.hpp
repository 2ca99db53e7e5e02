/*
 * GpuDustSimulation.hpp - the reference's dusty radiative transfer mode
 * (`CMacIonize --dusty-radiative-transfer --params FILE`,
 * DustSimulation::do_simulation, src/DustSimulation.cpp:67-186) on the GPU
 * engine: a SpiralGalaxyDensityFunction on the Cartesian grid, packets from
 * the SpiralGalaxyContinuousPhotonSource scattering off dust until they leave
 * the box, peel-off images of I, Q, U, saved as CCDImage::save does
 * (src/CCDImage.hpp:299-362).
 *
 * Parameters (names and defaults of the reference):
 *   dust:band                                 V (or K)
 *   CCDImage:view theta / view phi            89.7 degrees / 0. degrees
 *   CCDImage:image width / image height       200 / 200
 *   CCDImage:anchor x / anchor y              -12.1 kpc
 *   CCDImage:sides x / sides y                24.2 kpc
 *   CCDImage:type                             BinaryArray (or PGM)
 *   CCDImage:filename                         galaxy_image
 *   ContinuousPhotonSource:scale length stars / scale height stars /
 *     bulge over total ratio                  5. kpc / 0.6 kpc / 0.2
 *   DensityFunction:scale length ISM / scale height ISM / central density
 *                                             6. kpc / 0.22 kpc / 1. cm^-3
 *   DensityGrid:number of cells               [64, 64, 64]
 *   SimulationBox:anchor / sides / periodicity
 *   DustSimulation:number of photons          5e5
 *   DustSimulation:random seed                42
 *   DustSimulation:output folder              .
 * Beyond the reference, the galaxy at several inclinations from one run (the
 * views share the packets' walk, cmi_gpu_set_ccd_images; read only if the
 * key is there, 1 to CMI_GPU_MAX_VIEWS):
 *   CCDImage:number of views                  1
 * View 0 is described by the keys above; view k >= 1 by "view theta k" and
 * "view phi k" (required) and "anchor x k", "anchor y k", "sides x k",
 * "sides y k" (a missing one takes view 0's value). View 0 keeps its file
 * name, view k's is <filename>_view<k>.
 * A box that does not contain the origin (the galaxy's centre) is refused.
 * A periodic box is refused: the reference's integrate_optical_depth wraps
 * through a periodic face and never reaches the box edge
 * (src/CartesianDensityGrid.cpp:187-227,341).
 */
#ifndef CMI_GPUDUSTSIMULATION_HPP
#define CMI_GPUDUSTSIMULATION_HPP

#include "../../include/cmi_gpu.h"
#include "ImageWriter.hpp"
#include "ParameterFile.hpp"
#include "Plugins.hpp"

#include <chrono>
#include <cmath>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace cmi {

class GpuDustSimulation {
public:
  /* DustScattering's band constants, src/DustScattering.hpp:62-160 */
  struct Band {
    double g, p_l, albedo, kappa;
  };
  static Band band_constants(const std::string &band) {
    if (band == "V")
      return {0.44, 0.43, 0.54, 21.9};
    if (band == "K")
      return {0.02, 0.93, 0.21, 2.};
    throw ParameterError("Unknown band: " + band + "!");
  }

private:
  ParameterFile _params;
  SpiralGalaxyDensityFunction _density_function;
  SimulationBox _box;
  std::array<long long, 3> _ncell;
  long long _seed;
  double _r_stars, _h_stars, _bulge_over_total;
  std::string _band;
  Band _dust;
  std::string _output_folder;
  double _theta, _phi;
  long long _nx, _ny;
  double _image_anchor[2], _image_sides[2];
  std::string _image_type, _image_filename;
  long long _numphoton;
  /* several views: _views[0] repeats the members above */
  struct View {
    double theta, phi;
    double anchor[2], sides[2];
  };
  std::vector<View> _views;

public:
  /* the parameter reads of src/DustSimulation.cpp:79-116 and the
   * constructors they feed */
  explicit GpuDustSimulation(const std::string &parameterfile_name)
      : _params(parameterfile_name), _density_function(_params),
        _box(_params),
        _ncell(_params.get_integer_vector("DensityGrid:number of cells",
                                          {64, 64, 64})),
        _seed(_params.get_integer("DustSimulation:random seed", 42)),
        _r_stars(_params.get_physical_value(
            QUANTITY_LENGTH, "ContinuousPhotonSource:scale length stars",
            "5. kpc")),
        _h_stars(_params.get_physical_value(
            QUANTITY_LENGTH, "ContinuousPhotonSource:scale height stars",
            "0.6 kpc")),
        _bulge_over_total(_params.get_double(
            "ContinuousPhotonSource:bulge over total ratio", 0.2)),
        _band(_params.get_string("dust:band", "V")),
        _dust(band_constants(_band)),
        _output_folder(
            _params.get_string("DustSimulation:output folder", ".")),
        _theta(_params.get_physical_value(QUANTITY_ANGLE, "CCDImage:view theta",
                                          "89.7 degrees")),
        _phi(_params.get_physical_value(QUANTITY_ANGLE, "CCDImage:view phi",
                                        "0. degrees")),
        _nx(_params.get_integer("CCDImage:image width", 200)),
        _ny(_params.get_integer("CCDImage:image height", 200)),
        _image_anchor{_params.get_physical_value(
                          QUANTITY_LENGTH, "CCDImage:anchor x", "-12.1 kpc"),
                      _params.get_physical_value(
                          QUANTITY_LENGTH, "CCDImage:anchor y", "-12.1 kpc")},
        _image_sides{_params.get_physical_value(
                         QUANTITY_LENGTH, "CCDImage:sides x", "24.2 kpc"),
                     _params.get_physical_value(
                         QUANTITY_LENGTH, "CCDImage:sides y", "24.2 kpc")},
        _image_type(_params.get_string("CCDImage:type", "BinaryArray")),
        _image_filename(_params.get_string("CCDImage:filename",
                                           "galaxy_image")),
        _numphoton(
            _params.get_integer("DustSimulation:number of photons", 500000)) {
    /* CCDImage::get_type, src/CCDImage.hpp:96-106 */
    if (_image_type != "PGM" && _image_type != "BinaryArray")
      throw ParameterError("Unknown image type: " + _image_type + "!");
    if (_box.periodicity[0] || _box.periodicity[1] || _box.periodicity[2])
      throw ParameterError(
          "Periodic boxes are not supported in the dusty radiative transfer "
          "mode: the reference's optical depth integral never reaches the "
          "edge of a periodic box");
    /* SpiralGalaxyContinuousPhotonSource assumes a box centred on the origin
     * (src/SpiralGalaxyContinuousPhotonSource.hpp:112-113); away from it the
     * source's rejection loop would practically never end */
    for (int a = 0; a < 3; ++a)
      if (!(0. >= _box.anchor[a] && 0. < _box.anchor[a] + _box.sides[a]))
        throw ParameterError(
            "The simulation box must contain the origin: the spiral galaxy "
            "source is centred on it");
    if (_nx <= 0 || _ny <= 0 || _numphoton < 0)
      throw ParameterError("Bad image resolution or number of photons");
    /* (a key that is read shows in the used values: a file without the key
     * reads none of the new ones) */
    long long nviews = 1;
    if (_params.has_value("CCDImage:number of views"))
      nviews = _params.get_integer("CCDImage:number of views", 1);
    if (nviews < 1 || nviews > CMI_GPU_MAX_VIEWS)
      throw ParameterError("CCDImage:number of views must be 1.." +
                           std::to_string(CMI_GPU_MAX_VIEWS));
    _views.push_back({_theta, _phi, {_image_anchor[0], _image_anchor[1]},
                      {_image_sides[0], _image_sides[1]}});
    static const char *axis[2] = {"x", "y"};
    for (long long k = 1; k < nviews; ++k) {
      const std::string n = " " + std::to_string(k);
      View v = _views[0];
      const std::string kt = "CCDImage:view theta" + n;
      const std::string kp = "CCDImage:view phi" + n;
      if (!_params.has_value(kt))
        throw ParameterError(kt + " is required");
      if (!_params.has_value(kp))
        throw ParameterError(kp + " is required");
      v.theta = _params.get_physical_value(QUANTITY_ANGLE, kt, "0. degrees");
      v.phi = _params.get_physical_value(QUANTITY_ANGLE, kp, "0. degrees");
      for (int a = 0; a < 2; ++a) {
        const std::string ka = std::string("CCDImage:anchor ") + axis[a] + n;
        const std::string ks = std::string("CCDImage:sides ") + axis[a] + n;
        if (_params.has_value(ka))
          v.anchor[a] = _params.get_physical_value(QUANTITY_LENGTH, ka, "0. m");
        if (_params.has_value(ks))
          v.sides[a] = _params.get_physical_value(QUANTITY_LENGTH, ks, "1. m");
      }
      _views.push_back(v);
    }
  }

  /* the bulge-to-total ratio the source samples with
   * (src/SpiralGalaxyContinuousPhotonSource.hpp:109-114) */
  double corrected_bulge_over_total() const {
    const double kpc = 3.086e19;
    const double rC = 0.2 * kpc, rB = 2. * kpc, rJ = 0.4 * kpc;
    return _bulge_over_total * (1. - (rC / (rC + rJ)) / (rB / (rB + rJ)));
  }

  void describe(std::ostream &out) const {
    out.precision(17);
    out << "{\n  \"mode\": \"dusty-radiative-transfer\",\n";
    out << "  \"anchor\": [" << _box.anchor[0] << ", " << _box.anchor[1]
        << ", " << _box.anchor[2] << "],\n";
    out << "  \"sides\": [" << _box.sides[0] << ", " << _box.sides[1] << ", "
        << _box.sides[2] << "],\n";
    out << "  \"ncell\": [" << _ncell[0] << ", " << _ncell[1] << ", "
        << _ncell[2] << "],\n";
    out << "  \"number_of_photons\": " << _numphoton
        << ",\n  \"random_seed\": " << _seed << ",\n";
    out << "  \"dust\": {\"band\": \"" << _band << "\", \"g\": " << _dust.g
        << ", \"p_l\": " << _dust.p_l << ", \"albedo\": " << _dust.albedo
        << ", \"kappa\": " << _dust.kappa << "},\n";
    out << "  \"source\": {\"scale_length_stars\": " << _r_stars
        << ", \"scale_height_stars\": " << _h_stars
        << ", \"bulge_over_total\": " << _bulge_over_total
        << ", \"bulge_over_total_corrected\": " << corrected_bulge_over_total()
        << "},\n";
    out << "  \"density\": {\"central_density\": "
        << _density_function.central_density()
        << ", \"scale_length_ISM\": " << _density_function.scale_length()
        << ", \"scale_height_ISM\": " << _density_function.scale_height()
        << "},\n";
    out << "  \"image\": {\"theta\": " << _theta << ", \"phi\": " << _phi
        << ", \"width\": " << _nx << ", \"height\": " << _ny
        << ", \"anchor\": [" << _image_anchor[0] << ", " << _image_anchor[1]
        << "], \"sides\": [" << _image_sides[0] << ", " << _image_sides[1]
        << "], \"type\": \"" << _image_type << "\", \"filename\": \""
        << _image_filename << "\"}";
    /* (only with several views: one view is described as it always was) */
    if (_views.size() > 1) {
      out << ",\n  \"views\": [";
      for (size_t v = 0; v < _views.size(); ++v)
        out << (v ? ",\n    " : "\n    ") << "{\"theta\": " << _views[v].theta
            << ", \"phi\": " << _views[v].phi << ", \"anchor\": ["
            << _views[v].anchor[0] << ", " << _views[v].anchor[1]
            << "], \"sides\": [" << _views[v].sides[0] << ", "
            << _views[v].sides[1] << "], \"filename\": \""
            << view_filename(v) << "\"}";
      out << "\n  ]";
    }
    out << "\n}\n";
  }

  /* src/DustSimulation.cpp:118-186 */
  int run(int device, bool write_output, bool dry_run, bool verbose,
          bool do_describe) {
    const auto program_start = std::chrono::steady_clock::now();
    auto status = [verbose](const std::string &text) {
      if (verbose)
        std::cout << text << std::endl;
    };
    if (write_output) {
      const std::string pfilename =
          _output_folder + "/dust-parameters-usedvalues.param";
      std::ofstream pfile(pfilename);
      _params.print_contents(pfile);
      status("Wrote used parameters to " + pfilename + ".");
    }
    if (do_describe)
      describe(std::cout);
    if (dry_run) {
      status("Dry run requested. Program will now halt.");
      return 0;
    }

    cmi_gpu_config config;
    memset(&config, 0, sizeof config);
    for (int a = 0; a < 3; ++a) {
      config.anchor[a] = _box.anchor[a];
      config.sides[a] = _box.sides[a];
      config.ncell[a] = (int32_t)_ncell[a];
    }
    config.device = device;
    cmi_gpu_engine *engine = nullptr;
    check(cmi_gpu_create(&config, &engine), "cmi_gpu_create");
    struct Guard {
      cmi_gpu_engine *e;
      ~Guard() { cmi_gpu_destroy(e); }
    } guard{engine};

    /* DensityGrid::initialize: the density function at the cell midpoints
     * (src/CartesianDensityGrid.hpp:85-89) */
    status("Initializing DensityFunction...");
    const int64_t ncell = (int64_t)_ncell[0] * _ncell[1] * _ncell[2];
    std::vector<double> density(ncell), zero(ncell, 0.), ones(ncell, 1.);
    double cellside[3];
    for (int a = 0; a < 3; ++a)
      cellside[a] = _box.sides[a] / _ncell[a];
    struct Midpoint : public Cell {
      CoordinateVector x;
      double volume;
      CoordinateVector get_cell_midpoint() const override { return x; }
      double get_volume() const override { return volume; }
    };
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < ncell; ++i) {
      const int64_t idx[3] = {i / (_ncell[1] * _ncell[2]),
                              (i / _ncell[2]) % _ncell[1], i % _ncell[2]};
      Midpoint cell;
      for (int a = 0; a < 3; ++a)
        cell.x[a] = (_box.anchor[a] + cellside[a] * idx[a]) + 0.5 * cellside[a];
      cell.volume = cellside[0] * cellside[1] * cellside[2];
      density[i] = _density_function(cell).get_number_density();
    }
    check(cmi_gpu_upload_cells(engine, density.data(), zero.data(), nullptr),
          "upload_cells");
    check(cmi_gpu_upload_field(engine, CMI_GPU_FIELD_IONIC_FRACTION + 0,
                               ones.data()),
          "upload_field");
    status("Done.");

    check(cmi_gpu_set_dust_scattering(engine, _dust.g, _dust.p_l,
                                      _dust.albedo, _dust.kappa),
          "set_dust_scattering");
    if (_views.size() == 1) {
      check(cmi_gpu_set_ccd_image(engine, _theta, _phi, (int32_t)_nx,
                                  (int32_t)_ny, _image_anchor, _image_sides),
            "set_ccd_image");
    } else {
      std::vector<double> theta, phi, anchors, sides;
      for (const View &v : _views) {
        theta.push_back(v.theta);
        phi.push_back(v.phi);
        anchors.insert(anchors.end(), v.anchor, v.anchor + 2);
        sides.insert(sides.end(), v.sides, v.sides + 2);
      }
      check(cmi_gpu_set_ccd_images(engine, (int32_t)_views.size(),
                                   theta.data(), phi.data(), (int32_t)_nx,
                                   (int32_t)_ny, anchors.data(), sides.data()),
            "set_ccd_images");
    }
    check(cmi_gpu_set_continuous_source_spiral_galaxy(
              engine, _r_stars, _h_stars, _bulge_over_total),
          "set_continuous_source_spiral_galaxy");

    status("Start shooting " + std::to_string(_numphoton) + " photons...");
    const auto shoot_start = std::chrono::steady_clock::now();
    check(cmi_gpu_dust_shoot(engine, (uint32_t)_seed, 0, (uint64_t)_numphoton),
          "dust_shoot");
    check(cmi_gpu_synchronize(engine), "synchronize");
    const double shoot_seconds =
        std::chrono::duration<double>(std::chrono::steady_clock::now() -
                                      shoot_start)
            .count();
    status("Done shooting photons.");

    std::vector<double> image(_nx * _ny);
    for (size_t v = 0; v < _views.size(); ++v) {
      check(cmi_gpu_download_image_view(engine, (int32_t)v, image.data(),
                                        nullptr, nullptr),
            "download_image");
      if (write_output) {
        status("Saving final image...");
        save(image, 1. / (double)_numphoton, v);
        status("Done saving image.");
      }
    }
    const double total_seconds =
        std::chrono::duration<double>(std::chrono::steady_clock::now() -
                                      program_start)
            .count();
    status("Total program time: " + std::to_string(total_seconds) + " s.");
    status("Total photon shooting time: " + std::to_string(shoot_seconds) +
           " s.");
    return 0;
  }

private:
  static void check(int rc, const char *what) {
    if (rc != CMI_GPU_OK)
      throw std::runtime_error(std::string(what) + ": " +
                               cmi_gpu_last_error());
  }

  /* CCDImage::save, src/CCDImage.hpp:299-362 (ImageWriter.hpp) */
  void save(const std::vector<double> &image, double normalization,
            size_t view) const {
    (void)write_image(_output_folder + "/" + view_filename(view), _image_type,
                      image.data(), _nx, _ny, normalization);
  }

  /* view 0 keeps the file's name */
  std::string view_filename(size_t view) const {
    return view ? _image_filename + "_view" + std::to_string(view)
                : _image_filename;
  }
};

} // namespace cmi

#endif
