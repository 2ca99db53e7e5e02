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
 * Beyond the reference: the images, sky maps and absorption spectra of the
 * "EmissionImages:", "EmissionSkyMaps:" and "AbsorptionSpectra:" blocks.
 * EmissionSettings.hpp documents and reads their keys, EmissionProducts.hpp
 * renders what the first two ask for; do_simulation below is the order of
 * the whole run.
 */
#ifndef CMI_EMISSIVITYCALCULATIONSIMULATION_HPP
#define CMI_EMISSIVITYCALCULATIONSIMULATION_HPP

#include "EmissionProducts.hpp"
#include "Hdf5Reader.hpp"

namespace cmi {

class EmissivityCalculationSimulation {
  using Run = emission::Run;
  using Settings = emission::Settings;

  /* the state of the snapshot in SI units, in the file's order of rows until
   * reorder() */
  struct Snapshot {
    Hdf5Reader &file;
    double unit_length_in_SI = 1., unit_number_density_in_SI = 1.,
           unit_temperature_in_SI = 1., unit_time_in_SI = 1.;
    double abundances[6];
    size_t size = 0;
    std::array<long long, 3> ncell;
    std::vector<double> number_density, temperature, fractions;
    /* images: the real grid. cell_of_row[i] = the cell row i of the file
     * describes (its midpoint, with the box anchor as the origin); empty if
     * the run does not place the cells */
    std::array<double, 3> box_anchor = {0., 0., 0.}, box_sides = {1., 1., 1.};
    std::vector<size_t> cell_of_row;

    bool placed() const { return !cell_of_row.empty(); }

    Snapshot(Hdf5Reader &file, bool place) : file(file) {
      /* :101-117 */
      ParameterFile simulation_parameters;
      for (const auto &kv : file.open("/Parameters").attributes)
        simulation_parameters.add_value(kv.first,
                                        Hdf5Reader::as_string(kv.second));
      /* :123-147 */
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
        const auto it = units.attributes.find("Unit time in cgs (U_t)");
        if (it != units.attributes.end())
          unit_time_in_SI = Hdf5Reader::as_doubles(it->second).at(0);
      }
      /* :153-165: old parameter files name the abundances directly */
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
      read_cells(simulation_parameters);
      if (place)
        place_cells(simulation_parameters);
    }

    /* :209-229 */
    void read_cells(ParameterFile &simulation_parameters) {
      number_density = file.read_doubles("/PartType0/NumberDensity");
      temperature = file.read_doubles("/PartType0/Temperature");
      size = number_density.size();
      if (temperature.size() != size)
        throw ParameterError("snapshot with " + std::to_string(size) +
                             " densities and " +
                             std::to_string(temperature.size()) +
                             " temperatures");
      ncell = simulation_parameters.get_integer_vector(
          "DensityGrid:number of cells", {-1, -1, -1});
      if ((long long)size != ncell[0] * ncell[1] * ncell[2])
        throw ParameterError(
            "the snapshot does not hold DensityGrid:number of cells cells");
      fractions.resize((size_t)NUMBER_OF_IONNAMES * size);
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
    }

    /* the box of /Parameters and every row's cell in it */
    void place_cells(ParameterFile &simulation_parameters) {
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
          const long long k =
              (long long)std::floor(ncell[a] * p / box_sides[a]);
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

    /* cubes: the cells' velocities in the engine's cell order, [3][size];
     * empty for a field at rest */
    std::vector<double> cell_velocities(const emission::CubeSettings &cs,
                                        const std::string &block) const {
      std::vector<double> velocities;
      if (!cs.cubes || !placed() || cs.velocity_field == "Static")
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
    }

    /* the cells from the file's order into the engine's: every cell in its
     * place in the real box */
    void reorder() {
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
  };

  /* the engine with the snapshot's cells: on the real box if they are
   * placed; otherwise in the file's order on a device grid of the same shape
   * (every cell on its own: the shape only has to hold them) */
  static void create_engine(Run &run, const Snapshot &snap, int device) {
    cmi_gpu_config config = {};
    for (int a = 0; a < 3; ++a) {
      config.anchor[a] = snap.placed() ? snap.box_anchor[a] : 0.;
      config.sides[a] = snap.placed() ? snap.box_sides[a] : 1.;
      config.ncell[a] = (int32_t)snap.ncell[a];
    }
    config.device = device;
    if (cmi_gpu_create(&config, &run.engine) != CMI_GPU_OK)
      throw std::runtime_error(std::string("cmi_gpu_create: ") +
                               cmi_gpu_last_error());
    run.check(cmi_gpu_set_abundances(run.engine, snap.abundances));
    run.check(cmi_gpu_upload_cells(run.engine, snap.number_density.data(),
                                   snap.temperature.data(),
                                   snap.fractions.data()));
  }

  /* the flagged lines of every cell, [line][row of the file] */
  static std::vector<double>
  compute_emissivities(const Run &run, const Snapshot &snap,
                       const std::vector<int32_t> &lines) {
    const size_t size = snap.size;
    std::vector<double> values(lines.size() * size);
    if (!lines.empty())
      run.check(cmi_gpu_compute_emissivities(run.engine, (int32_t)lines.size(),
                                             lines.data(), 0, (int64_t)size,
                                             values.data()));
    if (!snap.placed())
      return values;
    /* the datasets keep the file's order */
    std::vector<double> in_rows(values.size());
    for (size_t k = 0; k < lines.size(); ++k)
      for (size_t i = 0; i < size; ++i)
        in_rows[k * size + i] = values[k * size + snap.cell_of_row[i]];
    return in_rows;
  }

  /* the AbsorptionSpectra: block */
  static void render_absorption(Run &run,
                                const emission::AbsorptionSettings &ab,
                                const std::vector<double> &velocities) {
    run.status("Rendering absorption spectra...");
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
    run.check(cmi_gpu_set_cell_velocities(
        run.engine, velocities.empty() ? nullptr : velocities.data()));
    run.check(cmi_gpu_render_absorption_spectra(
        run.engine, (int32_t)nl, ions.data(), weights.data(), S.data(),
        g.data(), ab.sigma_turb, (int64_t)nrays, ab.origins.data(),
        ab.directions.data(), ab.lengths.data(), ab.velocity.data(),
        (int32_t)ab.nchan, ab.vmin, ab.vmax, tau.data(), N.data()));
    if (!run.write_output)
      return;
    const std::string base = ab.folder + "/" + ab.prefix + "_absorption_";
    run.wrote(write_cube(base + "tau", tau.data(), (long long)nrays,
                         (long long)nl, ab.nchan));
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
                     (ab.lines[l]->wavelength / constants::lightspeed) * sum *
                         dv);
      }
    std::fclose(out);
    run.wrote(filename);
  }

  /* :181-193,258-263: the lines as datasets of /PartType0 (existing ones are
   * overwritten). Everything else in the file is carried over. */
  static void rewrite_snapshot(Hdf5Reader &file, const std::string &filename,
                               const std::vector<int32_t> &lines,
                               const std::vector<double> &values,
                               size_t size) {
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
            replaced = replaced || d.first == Settings::line_name(line);
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
      out.dataset("PartType0", Settings::line_name(lines[k]), {size},
                  [v, size](std::ostream &os) {
                    os.write(reinterpret_cast<const char *>(v), 8 * size);
                  });
    }
    const std::string temporary = filename + ".tmp";
    out.write(temporary);
    if (std::rename(temporary.c_str(), filename.c_str()) != 0)
      throw std::runtime_error("could not replace \"" + filename + "\"");
  }

public:
  /* EmissivityCalculationSimulation::do_simulation, :58-299 */
  static int do_simulation(const std::string &parameterfile_name,
                           const std::string &input_file_name, int device,
                           bool write_output, bool verbose,
                           bool describe = false) {
    ParameterFile params(parameterfile_name);
    const Settings settings(params);
    if (describe && settings.do_absorption) {
      settings.absorption.describe(std::cout);
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
    /* (the engine, once it is there, goes on every way out) */
    Run run(write_output, verbose);
    run.status("Reading file \"" + input_file_name + "\"...");
    Hdf5Reader file(input_file_name);
    const std::vector<int32_t> &lines = settings.lines;
    const bool views =
        (settings.do_images || settings.do_sky) && !lines.empty();
    Snapshot snap(file, views || settings.do_absorption);
    std::vector<double> velocities, sky_velocities, absorption_velocities;
    if (settings.do_images)
      velocities = snap.cell_velocities(settings.img, "EmissionImages");
    if (settings.do_sky)
      sky_velocities = snap.cell_velocities(settings.sky, "EmissionSkyMaps");
    if (settings.do_absorption)
      absorption_velocities =
          snap.cell_velocities(settings.absorption, "AbsorptionSpectra");

    run.status("Starting emissivity calculation...");
    std::vector<double> values;
    if (!lines.empty() || settings.do_absorption) {
      if (snap.placed())
        snap.reorder();
      create_engine(run, snap, device);
      values = compute_emissivities(run, snap, lines);
      if (views && settings.do_images) {
        emission::ParallelViews cam(settings.img, snap.box_anchor,
                                    snap.box_sides);
        emission::LymanAlpha lya{cam, snap.ncell, snap.box_sides, velocities,
                                 {}};
        emission::render_products(run, cam, lines, velocities,
                                  settings.img.lyman_alpha ? &lya : nullptr);
      }
      if (views && settings.do_sky) {
        emission::SkyObservers cam(settings.sky);
        emission::render_products(run, cam, lines, sky_velocities);
      }
      if (settings.do_absorption)
        render_absorption(run, settings.absorption, absorption_velocities);
      if (!run.written.empty())
        run.status("Wrote" + run.written + ".");
    }
    run.status("Finished emissivity calculation.");
    rewrite_snapshot(file, input_file_name, lines, values, snap.size);
    run.status("Closed file.");
    return 0;
  }
};

} // namespace cmi

#endif
