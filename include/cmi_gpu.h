/*
 * cmi_gpu.h - C ABI of the MI355X photoionization engine (libcmi_gpu.so).
 *
 * This is the drop-in boundary for ONE path of CMacIonize: photon-packet
 * transport through a regular Cartesian grid plus the per-cell ionization /
 * temperature balance, i.e. the body of the iteration loop of
 * IonizationSimulation::run (reference src/IonizationSimulation.cpp:359-643):
 *
 *     reset_grid -> shoot N packets -> [reduce] -> calculate_temperature
 *
 * Everything above that loop (parameter file, plugin objects, writers) stays
 * on the host; the plugins are lowered once, at initialisation, into the flat
 * descriptors passed through the cmi_gpu_set_* calls. Every entry point cites
 * the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - plain C types only: opaque handle, pointers and sizes;
 *  - every function returns 0 on success and a non-zero CMI_GPU_E* code on
 *    failure; cmi_gpu_last_error() gives the message (thread local). Nothing
 *    aborts (the reference's cmac_error aborts, src/Error.hpp:101-110);
 *  - "host" pointers are caller-owned host memory, copied during the call;
 *    "device" pointers are HIP device memory valid on the engine's device;
 *  - all quantities in SI units, fp64, ion order of src/ElementNames.hpp:101-154
 *    (H0 He0 C+ C2+ N0 N+ N2+ O0 O+ Ne0 Ne+ S+ S2+ S3+), cells row-major
 *    ix*ny*nz + iy*nz + iz (src/CartesianDensityGrid.hpp:137-144);
 *  - one host thread per handle; work is enqueued on the handle's HIP stream
 *    and is asynchronous unless stated otherwise.
 *  - there is no CPU fallback: without a HIP device cmi_gpu_create fails.
 */
#ifndef CMI_GPU_H
#define CMI_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMI_GPU_NION 14
#define CMI_GPU_NHEATING 2
#define CMI_GPU_NTYPE 4 /* src/PhotonType.hpp:36-50 */
/* mean-intensity + heating accumulators per cell (src/DensityGrid.hpp:150-197) */
#define CMI_GPU_NACC (CMI_GPU_NION + CMI_GPU_NHEATING)

enum {
  CMI_GPU_OK = 0,
  CMI_GPU_EINVAL = 1,   /* bad argument */
  CMI_GPU_EDEVICE = 2,  /* HIP runtime error / no device */
  CMI_GPU_ESTATE = 3,   /* call sequence error (e.g. shoot before sources) */
  CMI_GPU_ENOMEM = 4,
  /* the call did nothing and the caller runs its own path (SPH mappings) */
  CMI_GPU_EDECLINED = 5
};

/* field ids for upload / download / device pointers */
enum {
  CMI_GPU_FIELD_NUMBER_DENSITY = 0, /* IonizationVariables::_number_density */
  CMI_GPU_FIELD_TEMPERATURE = 1,    /* ::_temperature */
  CMI_GPU_FIELD_IONIC_FRACTION = 2, /* + ion (14 fields) ::_ionic_fractions */
  CMI_GPU_FIELD_MEAN_INTENSITY = 16, /* + ion (14 fields) ::_mean_intensity */
  CMI_GPU_FIELD_HEATING = 30,        /* + 0 (H), 1 (He)  ::_heating */
  CMI_GPU_NFIELD = 32
};

enum {
  CMI_GPU_SPECTRUM_MONOCHROMATIC = 0,
  CMI_GPU_SPECTRUM_PLANCK = 1,
  CMI_GPU_SPECTRUM_TABLE = 2 /* cmi_gpu_set_spectrum_table */
};
/* which PhotonSourceSpectrum of the run a table stands for
 * (src/IonizationSimulation.cpp:155-168: role "PhotonSourceSpectrum" of the
 * discrete sources, role "ContinuousPhotonSourceSpectrum") */
enum { CMI_GPU_ROLE_SOURCE = 0, CMI_GPU_ROLE_CONTINUOUS = 1 };
/* how a table is read between two of its samples: linearly, or linearly in
 * the logarithms (a power law through the two samples) */
enum { CMI_GPU_TABLE_LINEAR = 0, CMI_GPU_TABLE_LOGLOG = 1 };
enum { CMI_GPU_REEMIT_NONE = 0, CMI_GPU_REEMIT_PHYSICAL = 1,
       CMI_GPU_REEMIT_FIXED = 2 };

typedef struct cmi_gpu_engine cmi_gpu_engine;

/* Geometry of the CartesianDensityGrid (src/CartesianDensityGrid.cpp:40-95:
 * box anchor/sides, number of cells, periodicity flags) + engine options. */
typedef struct {
  double anchor[3];     /* SimulationBox:anchor (m) */
  double sides[3];      /* SimulationBox:sides (m) */
  int32_t ncell[3];     /* DensityGrid:number of cells */
  int32_t periodic[3];  /* SimulationBox:periodicity */
  int32_t device;       /* HIP device ordinal */
  /* 1: also accumulate the two heating integrals during transport. The
   * reference always does (src/DensityGrid.hpp:170-186); they are only used
   * by the temperature solve, so a run with "do temperature calculation:
   * false" may pass 0 and save two atomics per step. */
  int32_t track_heating;
  /* optional: HIP stream (hipStream_t) to enqueue on; NULL = own stream */
  void *stream;
  /* optional: caller-allocated device buffer for the CMI_GPU_NACC accumulator
   * fields, contiguous [CMI_GPU_NACC][ncell] doubles (so that the caller can
   * hand it to a collective, e.g. torch.distributed over RCCL); NULL = the
   * engine allocates it. The engine zeroes it at creation; in hydrogen-only
   * runs cmi_gpu_reset_grid clears only the fields such a run adds to (J_H,
   * the heating terms if tracked), so a caller that writes into the block
   * itself - other than sums of what engines wrote there - declares that
   * with cmi_gpu_set_tuning("accumulators_dirty", 1): the next reset then
   * clears the whole block (cmi_gpu_upload_field of an accumulator field
   * does the same by itself). */
  void *external_accumulators;
  /* optional domain decomposition (replaces DensitySubGridCreator's block
   * decomposition, src/DensitySubGridCreator.hpp:314-396): the engine holds
   * only the block of sub_ncell cells starting at cell sub_offset of the grid
   * described above; all zero = the whole grid. Every field, upload and
   * download of the engine then refers to the block's cells (row-major inside
   * the block). Packets that leave the block into another one are handed over
   * through cmi_gpu_set_export_buffer / cmi_gpu_shoot_flights. */
  int32_t sub_offset[3];
  int32_t sub_ncell[3];
} cmi_gpu_config;

/* ------------------------------------------------------------ lifetime -- */

/* replaces: DensityGridFactory::generate + CartesianDensityGrid ctor
 * (src/DensityGridFactory.hpp:73-77, src/CartesianDensityGrid.cpp:40-95) */
int cmi_gpu_create(const cmi_gpu_config *config, cmi_gpu_engine **engine);
int cmi_gpu_destroy(cmi_gpu_engine *engine);
const char *cmi_gpu_last_error(void);
/* blocks until all enqueued work is done */
int cmi_gpu_synchronize(cmi_gpu_engine *engine);
int64_t cmi_gpu_number_of_cells(const cmi_gpu_engine *engine);

/* ------------------------------------------------- plugin descriptors -- */

/* replaces: PhotonSourceDistribution::{get_number_of_sources, get_position,
 * get_weight, get_total_luminosity} as consumed by the PhotonSource ctor
 * (src/PhotonSourceDistribution.hpp:54-80, src/PhotonSource.cpp:60-146).
 * positions: host [n][3] (m); weights: host [n], must sum to 1 within 1e-9
 * (same check as the reference); total_luminosity in s^-1. n = 0 removes the
 * discrete sources (a run with a continuous source only). */
int cmi_gpu_set_sources(cmi_gpu_engine *engine, int32_t n,
                        const double *positions, const double *weights,
                        double total_luminosity);

/* replaces: ContinuousPhotonSource as consumed by the PhotonSource ctor and
 * get_random_photon (src/ContinuousPhotonSource.hpp,
 * src/PhotonSource.cpp:104-130,230-238). ISOTROPIC is
 * IsotropicContinuousPhotonSource on the simulation box
 * (src/IsotropicContinuousPhotonSource.hpp:95-191). luminosity (s^-1) is what
 * the PhotonSource ctor computes: get_total_luminosity(), or
 * get_total_surface_area() x the spectrum's get_total_flux(). With both kinds
 * of sources half of the packets come from each and the continuous ones carry
 * the weight L_continuous / L_discrete; all tallies (mean intensities, heating,
 * totweight, the per-type counts) are sums of weights, as in the reference. */
enum {
  CMI_GPU_CONTINUOUS_NONE = 0,
  CMI_GPU_CONTINUOUS_ISOTROPIC = 1,
  CMI_GPU_CONTINUOUS_PLANAR = 2
};
int cmi_gpu_set_continuous_source(cmi_gpu_engine *engine, int32_t type,
                                  double luminosity);
/* ... PlanarContinuousPhotonSource (src/PlanarContinuousPhotonSource.hpp:
 * 96-196): packets start on the rectangle [anchor, anchor + sides] (host [2],
 * along the two axes other than `axis`, in their natural order) of the plane
 * x[axis] = intercept, in an isotropic direction; it has its own luminosity
 * (has_total_luminosity()). */
int cmi_gpu_set_continuous_source_planar(cmi_gpu_engine *engine, int32_t axis,
                                         double intercept,
                                         const double *anchor,
                                         const double *sides,
                                         double luminosity);
/* the continuous source's PhotonSourceSpectrum (role
 * "ContinuousPhotonSourceSpectrum", src/IonizationSimulation.cpp:164-168) */
int cmi_gpu_set_continuous_spectrum_monochromatic(cmi_gpu_engine *engine,
                                                  double frequency);
int cmi_gpu_set_continuous_spectrum_planck(cmi_gpu_engine *engine,
                                           double temperature);

/* replaces: PhotonSourceSpectrum::get_random_frequency for
 * MonochromaticPhotonSourceSpectrum (src/MonochromaticPhotonSourceSpectrum.hpp:97-100) */
int cmi_gpu_set_spectrum_monochromatic(cmi_gpu_engine *engine,
                                       double frequency);
/* ... for PlanckPhotonSourceSpectrum (src/PlanckPhotonSourceSpectrum.cpp:53-113,149-165) */
int cmi_gpu_set_spectrum_planck(cmi_gpu_engine *engine, double temperature);

/* GENERIC LOWERING ("unknown plugin => sample the virtual on the
 * host into a table"). A PhotonSourceSpectrum, CrossSections or
 * RecombinationRates implementation that is known only through the
 * reference's virtual - a third-party plugin, or one of the reference's
 * data-file spectra - is evaluated by the host ONCE, at initialisation, on a
 * grid of its argument, and the device reads the table. The three entry
 * points below take such tables (host arrays, copied); host/Plugins.hpp's base
 * classes build them by default from the virtuals alone.
 *
 * replaces: PhotonSourceSpectrum::get_random_frequency
 * (src/PhotonSourceSpectrum.hpp:48-50) of ANY spectrum, given as its quantile
 * function: cumulative[n] strictly ascending from 0 to 1, frequency[n] (Hz)
 * the frequency below which that fraction of the photons lies. A packet draws
 * one uniform x, Utilities::locate finds its interval of cumulative[]
 * (src/Utilities.hpp:726-742) and the frequency is interpolated between the
 * interval's ends - CMI_GPU_TABLE_LINEAR as
 * src/HeliumTwoPhotonContinuumSpectrum.cpp:167-180 does, CMI_GPU_TABLE_LOGLOG
 * as src/PlanckPhotonSourceSpectrum.cpp:149-165 does. role: CMI_GPU_ROLE_*. */
int cmi_gpu_set_spectrum_table(cmi_gpu_engine *engine, int32_t role, int32_t n,
                               const double *frequency,
                               const double *cumulative,
                               int32_t interpolation);
/* replaces: CrossSections::get_cross_section (src/CrossSections.hpp:49-50) of
 * ANY implementation: frequency[n] (Hz, strictly ascending) and
 * sigma[14][n] (m^2; ion-major, the ions in the order of
 * src/ElementNames.hpp:101-154). Between two samples the cross section is
 * interpolated (CMI_GPU_TABLE_*; a log-log interval with a zero in it falls
 * back to linear), outside the table it keeps the end values: a jump at an
 * ionization threshold is two neighbouring samples. The run then carries all
 * 14 cross sections per packet, as with VernerCrossSections. */
int cmi_gpu_set_cross_sections_table(cmi_gpu_engine *engine, int32_t n,
                                     const double *frequency,
                                     const double *sigma,
                                     int32_t interpolation);
/* replaces: RecombinationRates::get_recombination_rate
 * (src/RecombinationRates.hpp:49) of ANY implementation: temperature[n] (K,
 * strictly ascending), alpha[14][n] (m^3 s^-1, indexed by the recombined
 * ion). */
int cmi_gpu_set_recombination_rates_table(cmi_gpu_engine *engine, int32_t n,
                                          const double *temperature,
                                          const double *alpha,
                                          int32_t interpolation);

/* replaces: CrossSections::get_cross_section for FixedValueCrossSections
 * (src/FixedValueCrossSections.hpp:151-154); sigma: host [14] (m^2) */
int cmi_gpu_set_cross_sections_fixed(cmi_gpu_engine *engine,
                                     const double *sigma);
/* ... for VernerCrossSections (src/VernerCrossSections.cpp:259-322) */
int cmi_gpu_set_cross_sections_verner(cmi_gpu_engine *engine);

/* replaces: RecombinationRates::get_recombination_rate for
 * FixedValueRecombinationRates (src/FixedValueRecombinationRates.hpp:157-160);
 * alpha: host [14] (m^3 s^-1), indexed by the recombined ion */
int cmi_gpu_set_recombination_rates_fixed(cmi_gpu_engine *engine,
                                          const double *alpha);
/* ... for VernerRecombinationRates (src/VernerRecombinationRates.cpp:140-333) */
int cmi_gpu_set_recombination_rates_verner(cmi_gpu_engine *engine);

/* replaces: Abundances (src/Abundances.hpp) as filled by
 * FixedValueAbundanceModel (src/FixedValueAbundanceModel.hpp:44-52);
 * abundances: host [6] = He, C, N, O, Ne, S relative to H */
int cmi_gpu_set_abundances(cmi_gpu_engine *engine, const double *abundances);

/* replaces: DiffuseReemissionHandlerFactory::generate
 * (src/DiffuseReemissionHandlerFactory.hpp:94-99): NONE, PHYSICAL
 * (src/PhysicalDiffuseReemissionHandler.cpp) or FIXED
 * (src/FixedValueDiffuseReemissionHandler.hpp, needs probability+frequency) */
int cmi_gpu_set_reemission(cmi_gpu_engine *engine, int32_t type,
                           double fixed_probability, double fixed_frequency);

/* replaces: TemperatureCalculator ctor parameters
 * (src/TemperatureCalculator.cpp:133-160) */
typedef struct {
  int32_t do_temperature_calculation; /* default 0 */
  int32_t minimum_number_of_iterations; /* 3 */
  double epsilon_convergence;           /* 1e-3 */
  int32_t maximum_number_of_iterations; /* 100 */
  double pah_heating_factor;            /* 0 */
  double cosmic_ray_heating_factor;     /* 0 */
  double cosmic_ray_heating_limit;      /* 0.75 */
  double cosmic_ray_heating_scale_length; /* 1.33333 kpc in m */
  double minimum_ionized_temperature;   /* 4000 K */
} cmi_gpu_temperature_params;
int cmi_gpu_set_temperature_params(cmi_gpu_engine *engine,
                                   const cmi_gpu_temperature_params *params);

/* ----------------------------------------------------------- cell data -- */

/* replaces: DensityGrid::set_densities / DensityGridInitializationFunction
 * (src/DensityGrid.cpp:40-62, src/DensityGrid.hpp:775-790): the host
 * evaluates DensityFunction::operator() per cell and uploads SoA arrays.
 * number_density, temperature: host [ncell]; ionic_fractions: host
 * [14][ncell] or NULL (= all zero). Synchronous. */
int cmi_gpu_upload_cells(cmi_gpu_engine *engine, const double *number_density,
                         const double *temperature,
                         const double *ionic_fractions);
/* single field, host [ncell]; synchronous */
int cmi_gpu_upload_field(cmi_gpu_engine *engine, int32_t field,
                         const double *values);
/* replaces: the DensityGrid iterator accessors a DensityGridWriter reads
 * (src/DensityGridWriter.hpp:96-124); host [ncell]; synchronous */
int cmi_gpu_download_field(cmi_gpu_engine *engine, int32_t field,
                           double *values);
/* device address of the first element of a field. State fields are [ncell]
 * contiguous doubles. The 16 accumulator fields (MEAN_INTENSITY+0..13,
 * HEATING+0..1) share ONE contiguous block of 16 * ncell doubles starting at
 * the pointer of MEAN_INTENSITY+0 - that block is what a multi-process caller
 * sum-reduces; inside it element (field f, cell c) is at
 * (this function's pointer for f) + c * cell_stride, with the strides reported
 * by cmi_gpu_accumulator_layout: [16][ncell] for hydrogen-only transport
 * (field f at f * field_stride); [ncell][16] when all ions are transported,
 * a cell's 16 values then in the order of their ionization thresholds - J of
 * H0 O0 N0, the hydrogen heating term, J of Ne0 S+ C+ N+ | J of He0, the
 * helium heating term, J of S++ O+ Ne+ S+++ N++ C++ - so that a photon below
 * 24.59 eV touches one 64-B line of the row, not two (field_stride 1 tells
 * the layout, not the field's offset: ask this function per field). */
/* (A pointer to a state field - n, T, a fraction - lets the caller read and
 * write the cells behind the engine's back: from this call on the engine
 * makes every ionic fraction in every update, tuning "defer_metals" or not.) */
void *cmi_gpu_field_device_pointer(cmi_gpu_engine *engine, int32_t field);
/* How the hydrogen-only update stands (any pointer may be NULL): whether
 * x[2..13] of the last update are still to be made, whether the padded
 * records of the transport are those of the cells as they are, whether a
 * whole-grid update of this engine may defer x[2..13] at all. */
int cmi_gpu_get_update_state(cmi_gpu_engine *engine, int32_t *metals_pending,
                             int32_t *pad_records_valid,
                             int32_t *deferral_allowed);
/* What the last call that transported new packets flew its first generation
 * with (any pointer may be NULL): the build - 0 the general kernel, 1 the
 * block table, 2 and 3 the padded march in its smaller and larger blocks, 4
 * the multi-ion kernel with the emission physics done ahead - and whether it
 * was the padded march's build for packets of one weight ("pad_uniform"). */
int cmi_gpu_get_transport_plan(cmi_gpu_engine *engine, int32_t *first_build,
                               int32_t *uniform_weight);
/* Whether that first generation flew the bundle build of the padded march
 * (tuning "bundle_march"): 1 or 0. cmi_gpu_get_transport_plan answers 2 for
 * either build of it. */
int cmi_gpu_get_bundle_march(cmi_gpu_engine *engine, int32_t *flown);
/* ... and whether it was the point build of the bundle build (tuning
 * "bundle_point"): 1 or 0; cmi_gpu_get_bundle_march answers 1 for it too. */
int cmi_gpu_get_bundle_point(cmi_gpu_engine *engine, int32_t *flown);
/* How the last launch of new packets got its order (any pointer may be
 * NULL): path - CMI_GPU_ORDER_NONE: the packets flew in the order of their
 * ids, _RADIX: key kernel and radix sort, _BUCKET: the bucket order (tuning
 * "bucket_order") -, the bits of the bucket order's two scatter levels, and
 * the packets that found their region or leaf full and fly, unordered, behind
 * the ordered ones (0 on the other paths). Asking for the overflow waits for
 * the engine's stream. */
#define CMI_GPU_ORDER_NONE 0
#define CMI_GPU_ORDER_RADIX 1
#define CMI_GPU_ORDER_BUCKET 2
int cmi_gpu_get_order_plan(cmi_gpu_engine *engine, int32_t *path,
                           int32_t *bits1, int32_t *bits2,
                           uint64_t *overflow);
int cmi_gpu_accumulator_layout(cmi_gpu_engine *engine, int64_t *field_stride,
                               int64_t *cell_stride);

/* ------------------------------------------------- the iteration body -- */

/* replaces: DensityGrid::reset_grid (src/DensityGrid.hpp:803-807) and zeroes
 * the packet counters (totweight, typecount, step counter) */
int cmi_gpu_reset_grid(cmi_gpu_engine *engine);

/* replaces: WorkDistributor::do_in_parallel(IonizationPhotonShootJobMarket) =
 * IonizationPhotonShootJob::execute for packets [first_packet, first_packet +
 * n_packets) of iteration `iteration` (src/IonizationSimulation.cpp:402,
 * src/IonizationPhotonShootJob.hpp:117-146). Packet p draws its random
 * numbers from Philox4x32-10(counter = {p, draw block}, key = {seed,
 * iteration}), so any partition of the packet range over calls / devices
 * gives the same packets. Accumulates into the mean-intensity (+heating)
 * fields and the counters. Asynchronous on the engine's stream without
 * re-emission; with re-emission passes (tuning reemit_passes = 1, the
 * default) the host reads the size of each generation's queue of re-emitted
 * packets back, so the call returns when the last generation is queued. */
int cmi_gpu_shoot(cmi_gpu_engine *engine, uint32_t seed, uint32_t iteration,
                  uint64_t first_packet, uint64_t n_packets);

/* ---- decomposed grids: the photon-buffer exchange of the task-based path
 * (PhotonTraversalTaskContext / MemorySpace / MPI photon buffers,
 * src/PhotonTraversalTaskContext.hpp:100-278). A flight that leaves the
 * engine's block into another block is appended to the export buffer as
 * CMI_GPU_FLIGHT_DOUBLES doubles:
 *   [0-2] origin, [3-5] direction, [6] path parameter, [7-9] next wall
 *   parameters, [10] optical depth left, [11] frequency,
 *   [12] int64: long index of the cell it enters, in the WHOLE grid,
 *   [13] 2 x uint32: packet id (relative to first_packet), rng position/type.
 * The caller moves the rows to the engine that owns that cell (any transport:
 * RCCL all-to-all, peer copies) and continues them there with
 * cmi_gpu_shoot_flights, which also follows their re-emissions and may export
 * again. The marcher's own state travels, so a packet's path lengths are
 * bit-identical to a run on the undivided grid. ---- */
#define CMI_GPU_FLIGHT_DOUBLES 16
/* device buffer [capacity][CMI_GPU_FLIGHT_DOUBLES] doubles, caller-owned
 * (device_rows == NULL: the engine allocates one of that capacity, for hosts
 * that exchange through host memory); resets the export count */
int cmi_gpu_set_export_buffer(cmi_gpu_engine *engine, void *device_rows,
                              uint64_t capacity);
/* flights exported since the last reset; fails with CMI_GPU_ENOMEM if more
 * left the block than the buffer holds. Synchronous. */
int cmi_gpu_get_export_count(cmi_gpu_engine *engine, uint64_t *count);
int cmi_gpu_reset_exports(cmi_gpu_engine *engine);
/* the same through host memory, for a host without a GPU-aware transport (the
 * reference's MPI photon buffers are host memory): copy the exported rows to
 * host_rows [capacity][CMI_GPU_FLIGHT_DOUBLES] (*count = their number) and
 * continue flights given in host memory. Synchronous copies. */
int cmi_gpu_download_exports(cmi_gpu_engine *engine, double *host_rows,
                             uint64_t capacity, uint64_t *count);
int cmi_gpu_shoot_flights_host(cmi_gpu_engine *engine, uint32_t seed,
                               uint32_t iteration, uint64_t first_packet,
                               const double *host_rows, uint64_t n_flights);
/* continue n_flights handed-over flights (device rows as above); seed,
 * iteration and first_packet as in the cmi_gpu_shoot call that emitted them */
int cmi_gpu_shoot_flights(cmi_gpu_engine *engine, uint32_t seed,
                          uint32_t iteration, uint64_t first_packet,
                          const void *device_rows, uint64_t n_flights);

/* replaces: IonizationPhotonShootJobMarket::update_counters
 * (src/IonizationSimulation.cpp:406): totweight and typecount[4] summed over
 * all shoot calls since the last reset; nsteps = number of cell crossings
 * (DDA steps) executed. Synchronous. Any pointer may be NULL. */
int cmi_gpu_get_counters(cmi_gpu_engine *engine, double *totweight,
                         double *typecount, uint64_t *nsteps);

/* number of atomic adds the transport kernels issued to the accumulator
 * fields since the last reset (diagnostic of the cross-lane aggregation) */
int cmi_gpu_get_atomic_count(cmi_gpu_engine *engine, uint64_t *natomics);

/* iterations of the transport kernel's march loop summed over all wavefronts
 * since the last reset: DDA steps / (64 x this) is the fraction of lanes that
 * did a step in an average iteration (diagnostic of the packet ordering) */
int cmi_gpu_get_wave_steps(cmi_gpu_engine *engine, uint64_t *nwavesteps);

/* EXPERIMENT ONLY (builds with -DCMI_EXPERIMENTS and the tuning key
 * "phase_stamps"; CMI_GPU_ESTATE otherwise): the stamps of the last
 * first-generation launch of a hydrogen-only table kernel. out[0..4]: shader
 * cycles the waves spent waiting at the flush point's first barrier, in the
 * flush, in the refill, in the march loop and at the end of flights;
 * out[5]: the 100 MHz clock when the first block started; out[6 + b]: when
 * block b left the kernel. *count: the values the launch wrote (6 + its
 * blocks); at most `capacity` are copied. Synchronous. */
int cmi_gpu_get_phase_clocks(cmi_gpu_engine *engine, uint64_t *out,
                             int64_t capacity, int64_t *count);

/* replaces: TemperatureCalculator::calculate_temperature(loop, totweight,
 * grid, block) (src/TemperatureCalculator.cpp:944-970), i.e. per cell either
 * IonizationStateCalculator::calculate_ionization_state
 * (src/IonizationStateCalculator.cpp:70-272) or the temperature solve
 * (src/TemperatureCalculator.cpp:567-931). Reads the (reduced) accumulators,
 * writes ionic fractions (+temperature) and the transport opacities.
 * Asynchronous for the ionization balance; the temperature solve runs as a
 * pipeline of kernels that reads one count back per secant step and returns
 * with the last kernel enqueued (tuning "temperature_pipeline"). */
int cmi_gpu_update_cells(cmi_gpu_engine *engine, uint32_t loop,
                         double totweight);
/* Rebuild the transport records {n x_H, n x_He} of all cells from the state
 * fields - after number density or the H / He neutral fractions were written
 * through cmi_gpu_field_device_pointer (e.g. by the gather that follows a
 * sharded cell update, src/IonizationSimulation.cpp:540-618).
 * Asynchronous. */
int cmi_gpu_refresh_transport_records(cmi_gpu_engine *engine);

/* the same for the cells [first_cell, first_cell + ncell) of the engine's
 * grid only - the `block` argument of
 * TemperatureCalculator::calculate_temperature: in the reference's MPI path
 * every rank solves its block of cells and the new state is gathered
 * (src/IonizationSimulation.cpp:532-618, MPICommunicator::distribute_block,
 * src/MPICommunicator.hpp:224-239). Asynchronous. */
int cmi_gpu_update_cells_range(cmi_gpu_engine *engine, uint32_t loop,
                               double totweight, int64_t first_cell,
                               int64_t ncell);

/* replaces: EmissivityCalculator::calculate_emissivities over a block of the
 * grid (src/EmissivityCalculator.cpp:126-430 per cell, :439-470 over the
 * grid; LineCoolingData::get_line_strengths, src/LineCoolingData.cpp:1859-1952,
 * and EmissivityCalculator::get_balmer_jump_emission, :42-116, under it).
 * lines[nlines] picks emission lines by their index in EmissivityValues
 * (src/EmissivityValues.hpp:36-81; CMI_GPU_NUMBER_OF_EMISSIONLINES of them),
 * emissivities[k * ncell + c] receives line lines[k] of cell first_cell + c
 * (J m^-3 s^-1; the avg_* entries are the reference's weights; all zero in a
 * cell with x_H >= 0.2 or T <= 3000 K, :134). Needs the abundances
 * (cmi_gpu_set_abundances) and a full-ion state; reads the cells as they are
 * on the device. Synchronous: returns with the host array filled. */
#define CMI_GPU_NUMBER_OF_EMISSIONLINES 42
int cmi_gpu_compute_emissivities(cmi_gpu_engine *engine, int32_t nlines,
                                 const int32_t *lines, int64_t first_cell,
                                 int64_t ncell, double *emissivities);

/* replaces: TrackerManager::add_trackers with SpectrumTrackers
 * (src/TrackerManager.hpp:178-205, src/SpectrumTracker.hpp:41-262) and the
 * hook in DensityGrid::update_integrals (src/DensityGrid.hpp:188-191): every
 * packet that crosses the cell holding positions[3 k ..] (with gas in it) is
 * counted in tracker k by frequency bin (nbins bins over [1, 4) x 3.289e15 Hz,
 * :88-90) and photon type (primary, diffuse H, diffuse He) - if
 * reference_directions[3 k ..] is not the null vector only packets within
 * opening_angles[k] (radians) of it (:178-186). At most 16 trackers; n = 0
 * removes them; opening_angles / reference_directions may be NULL (all
 * packets). Counting happens while enabled (the reference adds its trackers
 * for the last iteration, src/IonizationSimulation.cpp:367-370) and makes the
 * transport run without the combining table and without tile rounds - in the
 * exact marcher on an undivided grid, in the incremental one on a block of a
 * decomposed grid (flights handed over between blocks carry its state). */
int cmi_gpu_set_spectrum_trackers(cmi_gpu_engine *engine, int32_t n,
                                  const double *positions, int32_t nbins,
                                  const double *opening_angles,
                                  const double *reference_directions);
/* The same with a number of bins per tracker (nbins[n]: the reference's
 * trackers each have their own, `number of bins` in the block file) and a
 * kind per tracker (NULL: all spectrum trackers):
 * CMI_GPU_TRACKER_SPECTRUM as above, CMI_GPU_TRACKER_ABSORPTION an
 * AbsorptionTracker (src/AbsorptionTracker.hpp:49-235, the hook of
 * DensitySubGrid::update_intensity_counters, src/DensitySubGrid.hpp:592-617):
 * for every packet crossing the cell, path length x cross section x weight
 * per ion, summed by photon type - the cell's mean-intensity sums split by
 * type (m^3; cmi_gpu_get_tracker_absorption). The engine's cross sections
 * are the classic path's (no element abundance in them: the reference's
 * task-based packets carry A_element sigma, src/SourceDiscretePhotonTask
 * Context.hpp:172-180 - multiply the ion's column by its element's abundance
 * for that convention). An engine whose cross sections are FixedValue with
 * sigma = 0 for every ion but H0 runs the hydrogen-only kernels, which add
 * only the H0 column: the other thirteen are path length x 0 in the reference
 * as well. On a block of a decomposed grid a tracker outside
 * the block counts nothing; the caller adds the blocks' (and copies') counts
 * (TrackerManager::normalize merges copies, src/TrackerManager.hpp:307-318).
 *
 * CMI_GPU_TRACKER_WEIGHTED_SPECTRUM is a WeightedSpectrumTracker
 * (src/WeightedSpectrumTracker.hpp:44-446): every packet crossing the cell
 * adds 1 / (the area the unit cube shows along the packet's direction,
 * get_projected_area, :212-290) to the bin of its frequency, by photon type
 * (cmi_gpu_get_tracker_flux). Its nbins[k] bins are LinearFrequencyBins from
 * 13.6 eV to 54.4 eV (src/LinearFrequencyBins.hpp:80-88) until
 * cmi_gpu_set_tracker_frequency_bins says otherwise; opening angle and
 * reference direction are not used. */
#define CMI_GPU_TRACKER_SPECTRUM 0
#define CMI_GPU_TRACKER_ABSORPTION 1
#define CMI_GPU_TRACKER_WEIGHTED_SPECTRUM 2
int cmi_gpu_set_trackers(cmi_gpu_engine *engine, int32_t n,
                         const double *positions, const int32_t *kinds,
                         const int32_t *nbins, const double *opening_angles,
                         const double *reference_directions);
int cmi_gpu_enable_trackers(cmi_gpu_engine *engine, int32_t enable);
/* replaces: FrequencyBinsFactory::generate for a WeightedSpectrumTracker
 * (src/FrequencyBinsFactory.hpp:57-72, `FrequencyBins:type`).
 * CMI_GPU_FREQUENCY_BINS_LINEAR: the tracker's nbins bins between
 * minimum_frequency and maximum_frequency (Hz), lower frequencies counted in
 * the first bin and higher ones in the last (LinearFrequencyBins::
 * get_bin_number, src/LinearFrequencyBins.hpp:115-125).
 * CMI_GPU_FREQUENCY_BINS_LEVEL: one bin per ion, from its ionization energy
 * (src/ElementData.hpp:39-105) to the next higher one, the last up to four
 * times hydrogen's (src/LevelFrequencyBins.hpp:52-86; the tracker must have
 * been set with 14 bins; the two frequencies are not used). After
 * cmi_gpu_set_trackers, before packets fly. */
#define CMI_GPU_FREQUENCY_BINS_LINEAR 0
#define CMI_GPU_FREQUENCY_BINS_LEVEL 1
int cmi_gpu_set_tracker_frequency_bins(cmi_gpu_engine *engine, int32_t tracker,
                                       int32_t type, double minimum_frequency,
                                       double maximum_frequency);
/* The weighted trackers' sums since the trackers were set, tracker after
 * tracker: tracker k's at flux[4 first_k + type nbins_k + bin], first_k = the
 * bins of the trackers before it, type in the order of
 * src/PhotonType.hpp:36-50 (zero rows for the other kinds of tracker). Not
 * normalised (WeightedSpectrumTracker::normalize multiplies by luminosity /
 * total weight / the cell's side squared, :106-116). Synchronous. */
int cmi_gpu_get_tracker_flux(cmi_gpu_engine *engine, double *flux);
/* probe: WeightedSpectrumTracker::get_projected_area for n directions
 * ([n][3], unit vectors), evaluated on the host by the function the kernels
 * call (test/testWeightedSpectrumTracker.cpp's known answers) */
int cmi_gpu_projected_areas(const double *directions, int64_t n,
                            double *areas);
/* absorption[(k * 4 + type) * 14 + ion] since the trackers were set, type in
 * the order of src/PhotonType.hpp:36-50 (the row of PHOTONTYPE_ABSORBED stays
 * zero: no packet flies with that type). Not normalised
 * (AbsorptionTracker::normalize multiplies by luminosity / total weight).
 * Synchronous. */
int cmi_gpu_get_tracker_absorption(cmi_gpu_engine *engine,
                                   double *absorption);
/* The counts since the trackers were set, tracker after tracker: tracker k's
 * at counts[3 first_k + type nbins_k + bin], first_k = the bins of the
 * trackers before it (with one bin count for all: counts[(k * 3 + type) *
 * nbins + bin]; SpectrumTracker::output_tracker's three columns, :226-238).
 * Synchronous. */
int cmi_gpu_get_tracker_counts(cmi_gpu_engine *engine, uint64_t *counts);

/* ---- escape maps: the ionizing packets that leave the box, by direction ----
 * (no counterpart in the reference, whose trackers sit in cells.) A tally
 * sky[3][nfreq][nlon * nmu] of doubles on the device. While trackers are
 * enabled (cmi_gpu_enable_trackers: the one switch of the last iteration),
 * every packet whose flight ends because it has left the WHOLE box - the
 * packets cmi_gpu_get_counters counts in typecount[0..2] - adds its weight,
 * once, to
 *     sky[(type * nfreq + bin) * nlon * nmu + i * nmu + j]
 * type: 0 primary, 1 diffuse H I, 2 diffuse He I (src/PhotonType.hpp:36-50).
 * bin: that of the packet's frequency by the weighted spectrum tracker's
 *   FrequencyBins: CMI_GPU_FREQUENCY_BINS_LINEAR nfreq bins between
 *   minimum_frequency and maximum_frequency (Hz), frequencies outside in the
 *   first / last; CMI_GPU_FREQUENCY_BINS_LEVEL the 14 level bins (nfreq must
 *   be 14, the two frequencies are ignored).
 * (i, j): the pixel of the packet's direction of travel d on an equal-area
 *   grid in the frame e_1, e_2, e_3 - frame[9] holds them as rows, the sky
 *   maps' convention, orthonormal to 1e-9 -:
 *     mu = d . e_3,                    j = min(nmu - 1, floor((mu + 1) / 2 * nmu))
 *     l = atan2(d . e_2, d . e_1),     i = min(nlon - 1, floor((l + pi) / (2 pi) * nlon))
 *   Every pixel covers 4 pi / (nlon nmu) sr; a direction on an edge belongs to
 *   the pixel above it. The pixel says where a distant observer who receives
 *   the packet sits (in direction +d from the box), not a line of sight from
 *   inside. With an even nmu and e_3 a disc's normal the hemispheres separate
 *   exactly.
 * The unit is packet weight, not normalised: sky * luminosity / totweight is
 * photons s^-1 per pixel, bin and type. On a block of a decomposed grid a
 * hand-over to another block is no escape, and a periodic face is never
 * left; the blocks' arrays add up to the undivided grid's (the caller adds
 * them, over ranks too). While the tally counts, transport is routed as with
 * a tracker set: the exact marcher on an undivided grid, the incremental
 * marcher's tracker builds on a block; without it, or with trackers disabled,
 * nothing changes.
 * nlon == 0 removes the tally. CMI_GPU_EINVAL for a negative size, nmu or
 * nfreq < 1 with nlon > 0, 3 * nfreq * nlon * nmu > 2^24, level bins with
 * nfreq != 14, an empty linear range, a frame that is not orthonormal.
 * Setting zeroes the sums. */
int cmi_gpu_set_escape_tally(cmi_gpu_engine *engine, int32_t nlon, int32_t nmu,
                             const double frame[9], int32_t nfreq,
                             int32_t bins_type, double minimum_frequency,
                             double maximum_frequency);
/* zeroes the sums; CMI_GPU_ESTATE without a tally */
int cmi_gpu_reset_escape_tally(cmi_gpu_engine *engine);
/* sky[3 * nfreq * nlon * nmu] to the host. Synchronous. CMI_GPU_ESTATE without
 * a tally. */
int cmi_gpu_download_escape_tally(cmi_gpu_engine *engine, double *sky);
/* Host only: the kernel's binning function for n directions (unit vectors
 * directions[n][3] -> pixels[n] = i * nmu + j; either may be NULL with n = 0),
 * and / or the unit vectors centres[nlon * nmu][3] of the pixel centres
 * (mu = -1 + (2 j + 1) / nmu, l = -pi + 2 pi (i + 0.5) / nlon; NULL: not
 * wanted). CMI_GPU_EINVAL for nlon or nmu < 1 or a frame that is not
 * orthonormal. */
int cmi_gpu_escape_pixels(const double frame[9], int32_t nlon, int32_t nmu,
                          int64_t n, const double *directions, int32_t *pixels,
                          double *centres);
/* sigma[n][14] (m^2): the engine's configured cross sections (fixed, Verner or
 * table) at n frequencies (Hz), by the function the emission code uses, run on
 * the host. CMI_GPU_ESTATE before cross sections are set. */
int cmi_gpu_cross_sections(cmi_gpu_engine *engine, int64_t n,
                           const double *frequencies, double *sigma);

/* Performance knobs (no effect on what is computed, only on how):
 *   "sort_packets" (1)      process the packets of a launch in emission-
 *                           direction order, so that the lanes of a wave cross
 *                           the same cells
 *   "sort_tau_bits" (-1)    hydrogen-only transport: split every coarse
 *                           direction bin into 2^bits classes of the first
 *                           optical depth, so that the packets of a wave end
 *                           their flights at about the same step (0 = plain
 *                           direction order, -1 = chosen from the number of
 *                           packets per launch)
 *   "class_order" (-1)      with tau classes: 1 = the coarse direction bins of
 *                           odd index hold their classes the other way round,
 *                           so that neighbouring bins meet at equal classes
 *                           and no bundle mixes one bin's shortest flights
 *                           with the next one's longest; 0 = every bin from
 *                           the longest flights to the shortest; -1 = the
 *                           default of the run's kind (hydrogen-only: 1,
 *                           multi-ion: 0)
 *   "sort_dir_bits" (-1)    direction bits of the sort key, 2 .. 22 (an equal-area
 *                           2048 x 2048 lattice, Morton order); -1 = auto: 22,
 *                           or one or two fewer where that saves the radix
 *                           sort a pass
 *   "bucket_order" (1)      hydrogen-only launches on an undivided grid: the
 *                           order by two scatter levels - the first inside
 *                           the key kernel - and a sort of the leaves in LDS
 *                           instead of key kernel and radix sort; the same
 *                           order, word for word, unless a region or a leaf
 *                           overflows (cmi_gpu_get_order_plan). Taken where
 *                           the two levels leave at most 8 key bits to the
 *                           leaves; 0 = always the radix sort
 *   "bucket_min_packets" (1000000) launches of fewer packets keep the radix
 *                           sort
 *   "bucket_bits1", "bucket_bits2" (-1) bits of the two levels, 0 .. 8; -1 =
 *                           from the launch's packets, a mean leaf of 1024 to
 *                           2047 pairs (8 + 8 at 1e8 packets)
 *   "bucket_slack_permille" (-1) room of a region and a leaf beyond its mean
 *                           share of the launch, in thousandths; -1 = 12 and
 *                           9 standard deviations of a Poisson count (2 % and
 *                           23 % at 1e8 packets): uniform keys never overflow
 *   "aggregate" (2)         what happens to a step's contributions before
 *                           HBM sees an atomic: 0 = one atomic per lane and
 *                           step; 1 = lanes of a wave in the same cell are
 *                           summed first; 2 = + per-block combining table in
 *                           LDS, written back between ray bundles (hydrogen-only
 *                           transport; multi-ion transport uses its own
 *                           cooperative scheme for any value > 0)
 *   "aggregate_reemit" (0)  the same for the later re-emission passes
 *   "refill_threshold" (64) idle lanes of a wave that trigger a refill
 *   "chunk" (64)            consecutive packets a wave takes at a time
 *   "max_blocks_per_cu" (8), "max_packets_per_launch" (2^27)
 *   "reemit_passes" (1)     with diffuse re-emission: absorbed packets are
 *                           parked in a queue, a separate interaction kernel
 *                           decides about their re-emission and the survivors
 *                           fly in the next launch of the transport kernel
 *                           (keeps the primary ray bundles together and the
 *                           transport kernel small); 0 = follow re-emissions
 *                           in place
 *   "refill_threshold_reemit" (32), "reemit_inline_below" (-1 = auto: 4096, on a block of a decomposed grid 262144),
 *   "reemit_max_passes" (12)  refill threshold of the later passes; a pass
 *                           with fewer packets than this, or the last allowed
 *                           pass, follows re-emissions in place
 *   "tile_rounds" (1)       with re-emission in passes: the later generations
 *                           fly in tile rounds - flights wait in slots keyed by
 *                           the tile (16^3 cells; 8^3 for multi-ion transport)
 *                           they are about to enter; every round sorts the
 *                           slots and marches each flight through ONE tile
 *                           with the tile's transport records and accumulators
 *                           in LDS (written back with full-line atomics)
 *                           instead of one memory-side atomic per DDA step
 *   "tile_min_flights" (100000), "tile_min_per_item" (-1 = auto: 200)
 *                           the rounds end - and passes of the transport
 *                           kernel take over - once fewer flights than this,
 *                           or fewer than this per unit of work (<= 8192
 *                           flights of one tile), are left
 *   "tile_refill_threshold" (48)  idle lanes of a wave that trigger a refill
 *                           in the tile kernel
 *   "park_in_place" (1)     runs with re-emission in passes / tile rounds: the
 *                           first generation leaves an absorbed packet's
 *                           record at the place of its position in the
 *                           launch's order instead of claiming a place from
 *                           the queue's counter (one returning atomic per
 *                           bundle on one word)
 *   "tile_compact_ratio" (-1)  the rows of the live flights are copied into
 *                           fresh rows, in tile order, once the flights are
 *                           spread over this many slots per flight; 0: never;
 *                           -1: 2 for multi-ion transport, never for
 *                           hydrogen-only
 *   "temperature_pipeline" (1)  the temperature solve as one kernel per stage
 *                           of a secant step (ionization balance / line
 *                           cooling / update), each dense in like work -
 *                           0: one kernel holding the whole solve of a cell
 *   "temperature_finish_slots" (1024)  ... and once so few cells are still
 *                           iterating, one launch takes them to their end
 *                           (a wave per cell)
 *   "pad_march" (1)         hydrogen-only runs on a whole, non-periodic grid:
 *                           the first generation marches through a copy of
 *                           sigma_H n x_H with one layer of ghost cells, whose
 *                           record says that the packet has left the box (no
 *                           cell counters per axis in the march)
 *   "pad_uniform" (1)       ... and where every packet of the call carries one
 *                           weight (no continuous source beside the discrete
 *                           ones, or equal weights) and no heating term is
 *                           tracked, it sums path lengths and multiplies a
 *                           cell's sum by weight x sigma_H once (J_H equal up
 *                           to rounding, counters identical) - 0: a product
 *                           per step
 *   "xcd_remap" (0)         sorted first generation: the blocks that share an
 *                           XCD (block index mod 8) take neighbouring
 *                           positions of the packet order, so that bundles
 *                           crossing the same cells share one L2 (measured:
 *                           no difference on the benchmark grids)
 *   "pre_emission" (1)      multi-ion runs with sorted packets: the spectrum
 *                           sample, the 14 cross sections and the optical
 *                           depth of every new packet are computed by the
 *                           sort-key kernel and read back by the transport
 *                           kernel
 *   "defer_weights" (1)     multi-ion runs: the 14 cross sections of re-emitted
 *                           flights are computed by a kernel of their own, not
 *                           inside the re-emission kernels
 *   "tile_counting_sort" (1)  the slots are put in tile order by counting
 *                           (per-tile counters in LDS; up to 32768 tiles) -
 *                           0: by rocPRIM's radix sort
 *   "update_reuse" (1)      hydrogen-only cell update: the recombination rates
 *                           and charge transfer fits of the metals' balance
 *                           depend on the temperature alone; a wave keeps
 *                           those of one temperature and every row of 64
 *                           cells that all have it, bit for bit, reads them
 *                           (same results) - 0: every cell evaluates them
 *   "defer_metals" (1)      hydrogen-only update of the whole grid without a
 *                           temperature solve: x[2..13], which no kernel of
 *                           such a run reads, are made when somebody looks
 *                           (a download, the emissivities, a renderer, ...),
 *                           not in every iteration (same results, bit for
 *                           bit) - 0: by every update
 *   "update_writes_pad" (1) ... and that update writes the padded records
 *                           of the next transport step itself - 0: a pass of
 *                           its own in every cmi_gpu_shoot
 *   "timing" (0)            record HIP events around every launch for
 *                           cmi_gpu_get_timing / _kernel_timing /
 *                           _launch_times (off: a run creates no events)
 *   "exact_dda" (0)         march with the reference's per-step arithmetic
 *                           (bit-identical path lengths) instead of the
 *                           incremental marcher (equal up to rounding)
 *   "span_claim" (1)        first generation of the hydrogen-only runs that
 *                           use the block table: a block takes its packets a
 *                           span (one chunk per wave) at a time from a cursor
 *                           in device memory - one cursor per XCD with
 *                           "xcd_remap" - instead of a fixed share by block
 *                           index
 *   "emit_before_flush" (1) the same kernels: the refill ahead of the flush
 *                           point's barrier - a wave that arrives early emits
 *                           its next bundle while it would wait
 *   "class_group_chunks" (1) sorted launches with tau classes: the key's
 *                           coarse direction bins hold this many chunks of 64
 *                           packets per class (1 to 64) - with 8 the chunks of
 *                           one round of a block come from one class, or two
 *                           neighbouring ones, of a patch eight times as wide
 *   "bundle_march" (1)      the padded first generation of launches whose
 *                           every refill fills a whole idle wave - "chunk" 64,
 *                           "refill_threshold" 64, "span_claim", new packets
 *                           on an undivided grid of at most 2^25 cells, no
 *                           heating term, no re-emission -: the build of the
 *                           kernel made for exactly that (shoot_bundle_kernel;
 *                           the same packets in the same rounds) - 0: the
 *                           general kernel
 *   "bundle_point" (1)      such a launch whose packets all carry one weight
 *                           and come from ONE discrete source, with no
 *                           continuous source: the point build of that kernel
 *                           (shoot_bundle_kernel<true, true>: the refill reads
 *                           its arguments from a block on the device, only the
 *                           discrete source's emission is compiled, the start
 *                           cell and its walls are computed once per launch;
 *                           the same packets in the same rounds) - 0: the
 *                           bundle build
 *   "phase_stamps" (0)     EXPERIMENT ONLY: cmi_gpu_get_phase_clocks
 *   "exp_no_atomics" (0)    EXPERIMENT ONLY, builds with -DCMI_EXPERIMENTS
 *                           (results are wrong): 1 = skip the
 *                           accumulation; multi-ion kernels: 2 = post
 *                           destinations but skip the walk, 3 = walk without
 *                           the adds, 4 = as 2 without the table look-up,
 *                           5 = as 2 without the periodic write-backs,
 *                           6 = a quarter of the table adds
 * A host that cannot call this (the cmi-gpu executable, a code that links
 * the library mode) sets the environment variable
 * CMI_GPU_TUNING="key=value,key=value": cmi_gpu_create applies it to every
 * engine it makes (an unknown key makes it fail). For experiments and
 * bisections, not for configuration. */
int cmi_gpu_set_tuning(cmi_gpu_engine *engine, const char *key, int64_t value);

/* ------------------------------------------------- several GPUs, one host -- */

/* A group of engines driven by one host process, one per GPU of a node:
 * replicas of one grid, or the blocks of one decomposed grid. Replaces the
 * reference's MPICommunicator for this path (src/MPICommunicator.hpp); the
 * transport is RCCL over xGMI (loaded at the first reduce) and peer-to-peer
 * device writes. The engines stay owned by the caller.
 *
 * Engines of a group that hold the same cells form a CLASS: the replicas of
 * replica mode are one class; in domain mode several engines may hold the
 * same block - the reference's copies of a busy subgrid
 * (DensitySubGridCreator::create_copies, src/DensitySubGridCreator.hpp:437-531,
 * used for the subgrids that contain a source,
 * src/TaskBasedIonizationSimulation.cpp:514-560). cmi_gpu_group_create finds
 * the classes itself; copy r of c engines of a block emits the packets of
 * that block whose id is congruent to r modulo c and receives the flights of
 * those packets. The members of a class must sit on distinct devices (or all
 * on one: tests). */
typedef struct cmi_gpu_group cmi_gpu_group;
int cmi_gpu_group_create(int32_t n, cmi_gpu_engine *const *engines,
                         cmi_gpu_group **out);
int cmi_gpu_group_destroy(cmi_gpu_group *group);

/* replaces: the MPI_Allreduce(SUM) of every accumulator field after the
 * packets of all ranks have flown (src/IonizationSimulation.cpp:459-528,
 * MPICommunicator::reduce, src/MPICommunicator.hpp:504-560): afterwards every
 * engine of the (replica) group holds the sum over the group of the
 * accumulator fields a transport step can have written - ONE grouped
 * ncclAllReduce per contiguous piece instead of 16 chunked ones. The packet
 * counters are summed by the caller (cmi_gpu_get_counters of each engine).
 * Asynchronous on the engines' streams.
 * Also replaces DensitySubGridCreator::update_original_counters
 * (src/DensitySubGridCreator.hpp:556-574): the sum runs within every class
 * of the group, so in domain mode the copies of a block end with the block's
 * summed integrals - each then runs cmi_gpu_update_cells on identical input,
 * which stands in for update_copy_properties (:580-598). */
int cmi_gpu_group_reduce_accumulators(cmi_gpu_group *group);

/* replaces: the cell update of the reference's MPI path
 * (src/IonizationSimulation.cpp:532-618): every rank solves a block of the
 * cells (MPICommunicator::distribute, src/MPICommunicator.hpp:207-222), then
 * the temperature and the ionic fractions are gathered
 * (MPICommunicator::gather). Here per class of the group: member r solves
 * slab r of the class's cells (cmi_gpu_update_cells_range) and every member
 * ends with all slabs and their transport records - grouped in-place
 * ncclAllGathers over RCCL / xGMI between distinct devices; peer reads by a
 * kernel where the slabs are unequal or the engines share a device. A class
 * of one engine (a block without copies) simply updates its cells. Call after
 * cmi_gpu_group_reduce_accumulators. */
int cmi_gpu_group_update_cells(cmi_gpu_group *group, uint32_t loop,
                               double totweight);

/* replaces: the photon-buffer traffic between subgrids
 * (src/PhotonTraversalTaskContext.hpp:100-278, src/MemorySpace.hpp:96-127;
 * message format src/PhotonBuffer.hpp:46-48): one exchange round of a
 * decomposed grid whose blocks are the group's engines. Every flight in an
 * engine's export buffer is written into the inbox of the engine that owns
 * the cell it enters - by a kernel on the source device, across xGMI where
 * the owner is another GPU - the export buffers are emptied, and every engine
 * continues the flights it received (cmi_gpu_shoot_flights), which may export
 * again. *total_flights = flights handed over in this round; call until 0.
 * Only n x n counts cross the host. */
int cmi_gpu_group_exchange_flights(cmi_gpu_group *group, uint32_t seed,
                                   uint32_t iteration, uint64_t first_packet,
                                   uint64_t *total_flights);
/* What the exchange rounds cost on the HOST (the reference's counterpart is
 * the queue handling of src/TaskBasedIonizationSimulation.cpp:643-1073): over
 * the *rounds rounds that moved flights since the last reset, microseconds[0]
 * = until the n x n counts were known on the host, [1] = starting and joining
 * the owners' host threads beyond the longest cmi_gpu_shoot_flights call, [2]
 * = the whole of cmi_gpu_group_exchange_flights (with the flights). */
int cmi_gpu_group_exchange_stats(cmi_gpu_group *group, uint64_t *rounds,
                                 double *microseconds, int32_t reset);

/* --------------------------------------------------- test / measurement -- */

/* Parity probe of PhotonSource::get_random_photon + the first optical depth
 * (src/PhotonSource.cpp:208-249, src/IonizationPhotonShootJob.hpp:119-135)
 * for packets [first_packet, first_packet + n): host outputs position [n][3],
 * direction [n][3], frequency [n], cross_sections [n][14], tau [n].
 * Synchronous. */
int cmi_gpu_emit_packets(cmi_gpu_engine *engine, uint32_t seed,
                         uint32_t iteration, uint64_t first_packet, uint64_t n,
                         double *position, double *direction,
                         double *frequency, double *cross_sections,
                         double *tau);

/* Probe of the packet order: what a cmi_gpu_shoot of packets [first_packet,
 * first_packet + n) - one launch: n <= "max_packets_per_launch" - would fly
 * its first generation in, by the same plan and the same kernels. Host
 * outputs: out_ids [n] - position j of the launch is packet first_packet +
 * out_ids[j] -, out_keys [n] - the sort keys of those packets, in that order
 * (either may be NULL). cmi_gpu_get_order_plan then speaks of this launch.
 * CMI_GPU_ESTATE where such a call would not order its packets, or - a block
 * of a decomposed grid - orders a selection of them. Synchronous. */
int cmi_gpu_order_packets(cmi_gpu_engine *engine, uint32_t seed,
                          uint32_t iteration, uint64_t first_packet,
                          uint64_t n, uint32_t *out_ids, uint32_t *out_keys);

/* Parity probe of CartesianDensityGrid::interact
 * (src/CartesianDensityGrid.cpp:375-452) for n caller-specified packets:
 * position/direction host [n][3], tau host [n], sigma_H / sigma_He_corr host
 * [n] (the two cross sections that enter the optical depth). For packet i up
 * to max_steps (cell, ds) pairs are written to out_cell/out_ds
 * [n][max_steps]; out_nsteps [n]; out_last_cell [n] (-1 = left the box);
 * out_position [n][3] final position. Does NOT touch the accumulators.
 * Uses the marcher selected by the "exact_dda" tuning knob. Synchronous. */
int cmi_gpu_trace_packets(cmi_gpu_engine *engine, uint64_t n,
                          const double *position, const double *direction,
                          const double *tau, const double *sigma_H,
                          const double *sigma_He_corr, int32_t max_steps,
                          int64_t *out_cell, double *out_ds,
                          int32_t *out_nsteps, int64_t *out_last_cell,
                          double *out_position);

/* Parity probe of the spectrum samplers (get_random_frequency of
 * PlanckPhotonSourceSpectrum kind 0, HydrogenLymanContinuumSpectrum 1,
 * HeliumLymanContinuumSpectrum 2, HeliumTwoPhotonContinuumSpectrum 3): n
 * frequencies (Hz) at `temperature`, sample i from packet stream i of `seed`.
 * Synchronous. */
int cmi_gpu_sample_spectrum(cmi_gpu_engine *engine, int32_t kind,
                            double temperature, uint32_t seed, uint64_t n,
                            double *frequencies);

/* Parity probe of the thermal balance for n independent cells given as rows:
 * J [n][14] and heating [n][2] already normalised (jfac = hfac = 1),
 * temperature [n], number_density [n].
 * solve = 0: one TemperatureCalculator::compute_cooling_and_heating_balance
 *   (src/TemperatureCalculator.cpp:207-501) at the given temperature;
 *   out_pair [n][2] = {gain, loss}, out_fractions [n][14] = {h0, he0, metals};
 * solve = 1: TemperatureCalculator::calculate_temperature (:567-931);
 *   out_temperature [n], out_fractions [n][14], out_pair = heating terms.
 * Synchronous. */
int cmi_gpu_thermal_probe(cmi_gpu_engine *engine, int64_t n, int32_t solve,
                          const double *J, const double *heating,
                          const double *temperature,
                          const double *number_density, double *out_fractions,
                          double *out_temperature, double *out_pair);

/* Parity probe of the atomic-data functions for n input rows (host arrays),
 * so that the reference's own fixtures can be checked on the device:
 *  kind 0: in [n] frequency (Hz) -> out [n][14] CrossSections::
 *          get_cross_section (src/VernerCrossSections.cpp:259-322 or
 *          src/FixedValueCrossSections.hpp:151-154), m^2;
 *  kind 1: in [n] T (K) -> out [n][14] RecombinationRates::
 *          get_recombination_rate (src/VernerRecombinationRates.cpp:140-333),
 *          m^3 s^-1;
 *  kind 2: in [n][15] {T, n_e (m^-3), 13 abundances in the order of
 *          src/LineCoolingData.hpp:38-80} -> out [n] LineCoolingData::
 *          get_cooling (src/LineCoolingData.cpp:1767-1847);
 *  kind 3: in [n] T -> out [n][5] PhysicalDiffuseReemissionHandler::
 *          set_reemission_probabilities
 *          (src/PhysicalDiffuseReemissionHandler.hpp:66-105);
 *  kind 4: in [n] T / 1e4 K -> out [n][14][3] charge transfer: recombination
 *          with H, ionization by H+, recombination with He
 *          (src/ChargeTransferRates.cpp:44-157, :169-250, :262-395).
 * Synchronous. */
int cmi_gpu_physics_probe(cmi_gpu_engine *engine, int32_t kind, int64_t n,
                          const double *in, double *out);

/* Device time (HIP events on the engine's stream) spent in cmi_gpu_shoot
 * (packet ordering + every transport launch of a batch; shoot_launches counts
 * batches) and in the cell-update kernels since the last call with
 * reset != 0. Synchronous. */
int cmi_gpu_get_timing(cmi_gpu_engine *engine, int32_t reset,
                       double *shoot_ms, uint64_t *shoot_launches,
                       double *update_ms, uint64_t *update_launches);

/* Device time of the transport kernel alone (HIP events around each
 * shoot_kernel launch, one per re-emission generation) since the last
 * cmi_gpu_get_timing(reset != 0). Synchronous. */
int cmi_gpu_get_kernel_timing(cmi_gpu_engine *engine, double *kernel_ms,
                              uint64_t *kernel_launches);
/* the same per launch, in launch order: duration and the number of flights
 * the launch started (packets of the batch, then of each re-emission
 * generation). *count receives the number of launches; at most `capacity`
 * entries are written. Synchronous. */
int cmi_gpu_get_launch_times(cmi_gpu_engine *engine, uint64_t capacity,
                             double *ms, uint64_t *packets, uint64_t *count);
/* ... and the value of the DDA step counter (cmi_gpu_get_counters' nsteps:
 * steps since the last cmi_gpu_reset_grid) after each of those launches: the
 * steps a launch executed are the difference to the entry before. Needs
 * "timing". Synchronous. */
int cmi_gpu_get_launch_steps(cmi_gpu_engine *engine, uint64_t capacity,
                             uint64_t *steps, uint64_t *count);

/* ------------------------------------------ dusty radiative transfer -- */
/* The reference's other mode on the Cartesian grid, `--dusty-radiative-
 * transfer` (DustSimulation::do_simulation, src/DustSimulation.cpp:67-186):
 * packets from a spiral galaxy source scatter off dust (Henyey-Greenstein
 * phase function with Stokes parameters) until they leave the box; after
 * every scattering a peel-off towards the observer adds I, Q, U to a CCD
 * image. The grid is the engine's (cmi_gpu_create, not periodic, not a block
 * of a decomposed grid); the densities come through cmi_gpu_upload_cells,
 * whose number density is the dust's mass density (kg m^-3) and whose x_H is
 * 1 (src/SpiralGalaxyDensityFunction.hpp:116-130). The march reads
 * n kappa x_H per cell. Packet i draws from the stream (seed, iteration 0,
 * packet i) in the order csrc/device_dust.h lists. */

/* replaces: the DustScattering ctor (src/DustScattering.hpp:171-185, bands
 * V / K :94-160): HG asymmetry g, peak linear polarisation p_l, albedo and
 * the dust attenuation coefficient kappa (m^2 kg^-1); sc = 1, pc = 0 */
int cmi_gpu_set_dust_scattering(cmi_gpu_engine *engine, double g, double p_l,
                                double albedo, double kappa);

/* The same phase function constants for dust that follows the gas: the march
 * reads n sigma per cell, sigma in m^2 per hydrogen nucleus, and x_H is not
 * read - the k = n_H sigma_dust of cmi_gpu_render_line_images. sigma = 0 is
 * allowed (direct light only); a negative sigma is CMI_GPU_EINVAL. The later
 * of the two setters holds. */
int cmi_gpu_set_dust_scattering_per_hydrogen(cmi_gpu_engine *engine, double g,
                                             double p_l, double albedo,
                                             double sigma);

/* replaces: the CCDImage ctor (src/CCDImage.hpp:123-160): view angles theta,
 * phi (radians), resolution nx x ny, image anchor[2] and sides[2] (m). The
 * image is I, Q, U of nx x ny pixels, pixel (ix, iy) at ix * ny + iy
 * (src/CCDImage.hpp:242-270). A new call replaces and clears the image. The
 * new image is allocated before anything of the engine changes: a call that
 * fails - CMI_GPU_EINVAL, or CMI_GPU_ENOMEM if the image does not fit into
 * the device's memory - leaves the camera selected before, and its image, as
 * they were. */
int cmi_gpu_set_ccd_image(cmi_gpu_engine *engine, double theta, double phi,
                          int32_t nx, int32_t ny, const double *anchor,
                          const double *sides);

/* replaces: the SpiralGalaxyContinuousPhotonSource ctor
 * (src/SpiralGalaxyContinuousPhotonSource.hpp:98-150): disc scale length and
 * height (m) and the bulge-to-total ratio (corrected for the cut-off bulge
 * centre as the reference does); the 1001-point disc CDF out to 1.2 x
 * |box anchor| is built here. The box is the engine's and must contain the
 * origin: the reference's sampler assumes a box centred on it (:112-113) and
 * its rejection loop would practically never end otherwise (CMI_GPU_EINVAL).
 * A packet whose source finds no position in the box in 1e6 attempts is
 * dropped and counted; cmi_gpu_download_image then fails. */
int cmi_gpu_set_continuous_source_spiral_galaxy(cmi_gpu_engine *engine,
                                                double r_stars, double h_stars,
                                                double bulge_over_total);

/* The cell-luminosity source (no counterpart in the reference): packets of
 * cmi_gpu_dust_shoot and cmi_gpu_dust_probe start inside the cells, cell c
 * with a probability proportional to a weight w_c >= 0 (W m^-3), at a
 * uniform position in it, in an isotropic direction, with Stokes (1, 0, 0,
 * 0); their life from the direct light on is the galaxy source's packets'.
 * The weights are the emissivity of emission line `line` (numbered as in
 * cmi_gpu_compute_emissivities) of the cells as they are, computed on the
 * device, or the caller's field[ncell] in the engine's cell order.
 * The sampling tables, over blocks of 256 consecutive cells (the last may be
 * partial): cell_sums[c], the running sum of w within c's block, cell by cell
 * from 0 in every block; block_sums[b], the running sum of the block totals,
 * block by block. One uniform u gives t = u block_sums[last]: the block is
 * the first with block_sums[b] > t, the cell the first of it with
 * cell_sums[k] > t - block_sums[b - 1] (csrc/device_dust.h has what happens
 * when rounding leaves none, and why a cell with w = 0 is never chosen).
 * A weight that is negative or not finite is CMI_GPU_EINVAL; weights that
 * sum to 0 are CMI_GPU_ESTATE ("nothing emits"); a line source needs the
 * abundances and the cell data as cmi_gpu_compute_emissivities does;
 * periodic boxes and blocks of a decomposed grid are refused. A call that
 * fails leaves no cell source. A later
 * cmi_gpu_set_continuous_source_spiral_galaxy selects the galaxy again.
 * A line source's tables are stale once the cells change (cmi_gpu_upload_
 * cells, an upload of a state field, a cell update): the next shoot or probe
 * fails with CMI_GPU_ESTATE until the source is set again. A field source
 * does not depend on the cells. Synchronous. */
int cmi_gpu_set_cell_source_line(cmi_gpu_engine *engine, int32_t line);
int cmi_gpu_set_cell_source_field(cmi_gpu_engine *engine, const double *field);

/* The cell source as built: its total luminosity V_cell block_sums[last]
 * (W) - an unnormalised image x total / (packets x pixel area) is in W m^-2
 * sr^-1 - and the tables: block_sums host [ceil(ncell / 256)], cell_sums
 * host [ncell]. Any of the three may be NULL. */
int cmi_gpu_get_cell_source(cmi_gpu_engine *engine, double *total_luminosity,
                            double *block_sums, double *cell_sums);

/* replaces: DustPhotonShootJob::execute for packets [first_packet,
 * first_packet + n) (src/DustPhotonShootJob.hpp:107-164), adding to the
 * image, accumulating. The first launch takes 2^14 packets; each later one
 * is sized from the DDA steps per packet measured so far to about 2^29 steps
 * (between 64 and 2^20 packets), so the call waits for every launch but the
 * last, which it leaves enqueued. A launch of a medium so dense that 64
 * packets take more than 2^29 steps still runs longer: its bound is 64
 * packets x 1e5 scatterings. A packet is stopped after 100000 scatterings and
 * counted (the reference has no cap); cmi_gpu_download_image then fails.
 * Periodic boxes are refused. */
int cmi_gpu_dust_shoot(cmi_gpu_engine *engine, uint32_t seed,
                       uint64_t first_packet, uint64_t n);

/* replaces: the image buffers of CCDImage (src/CCDImage.hpp:60-70) as
 * CCDImage::save reads them (:299-362), unnormalised. I, Q, U: host
 * [nx * ny] each, any of them may be NULL. Synchronous; fails if a packet
 * reached the scattering cap, or found no source position, since the last
 * reset. */
int cmi_gpu_download_image(cmi_gpu_engine *engine, double *I, double *Q,
                           double *U);
/* replaces: CCDImage::reset (src/CCDImage.hpp:226-232); also clears the
 * dust counters. Synchronous. */
int cmi_gpu_reset_image(cmi_gpu_engine *engine);

/* counters since the last reset: counters[6] = {DDA steps of both marches,
 * scatterings, packets stopped at the scattering cap, fp64 atomics into the
 * image, packets, packets the source found no position for}. Synchronous. */
int cmi_gpu_get_dust_counters(cmi_gpu_engine *engine, uint64_t *counters);

/* Parity probes of the device functions (synchronous, in launches of 2^14
 * rows); row k uses the random stream of packet first_packet + k with the
 * given seed. Rows, fp64:
 *  0 EMIT (src/DustPhotonShootJob.hpp:113-125): out {pos[3], dir[3]}, NaN if
 *    the source found no position
 *  1 SCATTER (src/DustScattering.cpp:41-323): in {dir[3], sin theta,
 *    cos theta, phi, sin phi, cos phi, I, Q, U, V}; out the same after
 *  2 SCATTER_TOWARDS (src/DustScattering.cpp:325-518): in as 1; out
 *    {hgfac, I, Q, U, V}
 *  3 OPTICAL_DEPTH (src/CartesianDensityGrid.cpp:328-363): in {pos[3],
 *    dir[3]}; out {tau, steps, first max_events cells}
 *  4 TRACE (src/DustPhotonShootJob.hpp:107-164): out {events, scatterings,
 *    steps, capped (either cap), rows[max_events] of {pos[3], I, Q, U, V,
 *    weight}}: the
 *    direct light (Stokes 1, 0, 0, 0, weight 0.25 exp(-tau) / pi), then
 *    each peel-off
 *  5 CELL_SOURCE (the cell source must be selected): out {cell, pos[3],
 *    dir[3]}
 *  6 SKY_PEEL (the sky camera must be selected, CMI_GPU_ESTATE otherwise):
 *    one peel-off of cmi_gpu_set_sky_camera's contract. in {pos[3], dir[3],
 *    sin theta, cos theta, phi, sin phi, cos phi, I, Q, U, V}; out {hgfac,
 *    I, Q, U, V after the rotation to the frame's pole, r, tau to the
 *    observer, steps, pixel}; pixel is -1 outside the map's window and -2
 *    inside the exclusion radius (everything but r is then 0)
 * EMIT and TRACE follow the selected source (a cell source always finds a
 * position). TRACE follows the selected camera as well: with the sky camera
 * a row's weight is the addend W / r^2 and its Stokes vector the rotated
 * one; an event inside the exclusion radius gives a row of its position and
 * zeros, and with the direct light switched off a packet's rows start at its
 * first peel-off. */
int cmi_gpu_dust_probe(cmi_gpu_engine *engine, int32_t kind, uint32_t seed,
                       uint64_t first_packet, int64_t n, const double *in,
                       double *out, int32_t max_events);

/* The sky camera: the peel-offs of cmi_gpu_dust_shoot go to an observer at
 * `origin` (m), inside or near the box, into an equirectangular map of I, Q,
 * U: nlon x nlat pixels over [lon_min, lon_max] x [lat_min, lat_max]
 * (radians) in the frame e_1, e_2, e_3 = the rows of frame[9], pixel (i, j)
 * at i * nlat + j - the pixels of cmi_gpu_render_line_sky_map below. The
 * call allocates and clears the image and selects this camera; a later
 * cmi_gpu_set_ccd_image selects the parallel camera again (and this call
 * replaces that one's image): cmi_gpu_dust_shoot, cmi_gpu_download_image
 * ([nlon * nlat] per Stokes parameter), cmi_gpu_reset_image and
 * cmi_gpu_get_dust_counters work on whichever camera was set last. Only the
 * cell source has this camera: a shoot or probe with the spiral galaxy
 * selected is CMI_GPU_ESTATE.
 * The camera draws no random number: a packet's emission, optical depths and
 * scatterings are those of the parallel camera for the same seed and id. Per
 * event - the direct light at the emission point (skipped, with its march, if
 * direct_light is 0), then every peel-off at a scattering point p:
 *   v = origin - p, r2 = v . v, r = sqrt(r2), k = v / r (a division per
 *   axis); the march uses 1 / k per axis.
 *   r2 < exclusion_radius^2: the event adds nothing and is counted.
 *   Optical depth to the observer, not to the box edge: the march of 3
 *   OPTICAL_DEPTH from p along k with the travelled length s summed step by
 *   step; the step with s + ds >= r adds (r - s) kappa and ends it. Towards
 *   an observer outside the box the march leaves the grid first.
 *   Scattering towards k: 2 SCATTER_TOWARDS with the observer's angles from
 *   k: cos theta = k_z, sin theta = sqrt(max(1 - k_z^2, 0)), phi =
 *   atan2(k_y, k_x) (0 where sin theta == 0), the skew in degrees.
 *   Q and U come out referred to the meridian through k and the grid's z
 *   axis. Unless e_3 is exactly (0, 0, 1) they are rotated to the meridian
 *   through e_3 by twice the angle chi from N_z = z - (z . k) k to N_e =
 *   e_3 - (e_3 . k) k (cos chi their normalised dot product, sin chi their
 *   normalised triple product with k, chi = 0 where either vanishes):
 *   Q' = Q cos 2 chi - U sin 2 chi, U' = Q sin 2 chi + U cos 2 chi.
 *   Pixel of the sky direction n = -k: l = atan2(n . e_2, n . e_1), b =
 *   asin(clamp(n . e_3)); x = l - lon_min wrapped into [0, 2 pi), inside if
 *   x < lon_max - lon_min; y = b - lat_min, inside if 0 <= y <= lat_max -
 *   lat_min; i = (int)(nlon x / width), j likewise, each clamped to its last
 *   index (rounding just below the far edge; b == lat_max is in the last
 *   row). Events outside the window are counted.
 *   Addend: W / r2 times (I, Q, U), W = 0.25 exp(-tau) / pi for the direct
 *   light and weight hgfac albedo exp(-tau) for a peel-off, the parallel
 *   camera's weights; fp64 atomics, zero terms skipped.
 * An unnormalised image x L_total / (packets x omega_ij), omega_ij the
 * pixel's solid angle (cmi_gpu_sky_map_directions), is in W m^-2 sr^-1.
 * CMI_GPU_EINVAL, nothing allocated or launched: an origin that is not
 * finite; a frame not orthonormal to 1e-9; not lon_min < lon_max <= lon_min
 * + 2 pi (an event must land in one pixel); latitudes as in
 * cmi_gpu_render_line_sky_map; nlon, nlat < 1 or nlon nlat > 2^28; an
 * exclusion radius that is negative or not finite, or 0 with the origin in
 * the closed box (the estimator's variance diverges at r -> 0 and an event
 * at r = 0 would add infinity). CMI_GPU_ENOMEM if the map does not fit into
 * the device's memory; like a refused call it leaves the camera selected
 * before, and its image, as they were (the map is allocated before anything
 * of the engine changes). Synchronous. */
int cmi_gpu_set_sky_camera(cmi_gpu_engine *engine, const double origin[3],
                           const double frame[9], double lon_min,
                           double lon_max, double lat_min, double lat_max,
                           int32_t nlon, int32_t nlat, double exclusion_radius,
                           int32_t direct_light);

/* A validation helper, not part of a run: the argument checks of
 * cmi_gpu_set_sky_camera for a box (host only, no engine, no device), so
 * that drivers and tests can check a camera before an engine exists:
 * CMI_GPU_OK or CMI_GPU_EINVAL with the message that call would give */
int cmi_gpu_check_sky_camera(const double box_anchor[3],
                             const double box_sides[3], const double origin[3],
                             const double frame[9], double lon_min,
                             double lon_max, double lat_min, double lat_max,
                             int32_t nlon, int32_t nlat,
                             double exclusion_radius);

/* counters[2] = {events inside the exclusion radius, events outside the
 * map's window} since the last reset. Synchronous. */
int cmi_gpu_get_sky_camera_counters(cmi_gpu_engine *engine,
                                    uint64_t *counters);

/* Several cameras in one run: views that share the packets' random walk (no
 * counterpart in the reference). The cameras above draw no random number, so
 * a packet's emission, optical depths and scatterings do not depend on the
 * camera: with K views cmi_gpu_dust_shoot walks each packet once and repeats
 * only the events - at the direct light and at every scattering, for the
 * views 0..K-1 in this order, the event of the single camera set with view
 * v's arguments, with its expressions in its order. View v's image is thus
 * the single camera's image of the same seed and packets but for the order
 * in which the atomics add, and the views of one run share their noise. A
 * run holds cameras of one kind: K parallel views (cmi_gpu_set_ccd_images) or
 * K point observers (cmi_gpu_set_sky_cameras). */
#define CMI_GPU_MAX_VIEWS 64

/* K = nviews CCD images of the shared resolution nx x ny: view v looks along
 * (theta[v], phi[v]) (radians) with the image anchors[2 v + {0, 1}] and
 * sides[2 v + {0, 1}] (m), as cmi_gpu_set_ccd_image's arguments. Allocates and
 * clears the stack [nviews][3][nx * ny] and selects these views; a later
 * cmi_gpu_set_ccd_image or cmi_gpu_set_sky_camera selects that single camera
 * again, and this call replaces theirs. CMI_GPU_EINVAL, with nothing
 * allocated and the camera selected before left as it was: nviews outside
 * [1, CMI_GPU_MAX_VIEWS], or a view that cmi_gpu_set_ccd_image would refuse
 * (the message names the first such view); CMI_GPU_ENOMEM, likewise, if the
 * stack does not fit into the device's memory. Synchronous. */
int cmi_gpu_set_ccd_images(cmi_gpu_engine *engine, int32_t nviews,
                           const double *theta, const double *phi, int32_t nx,
                           int32_t ny, const double *anchors,
                           const double *sides);

/* K = nviews sky cameras that share the window, the resolution and
 * direct_light: observer v at origins[3 v + a] with the frame frames[9 v + j]
 * and the exclusion radius exclusion_radii[v], as cmi_gpu_set_sky_camera's
 * arguments. The stack is [nviews][3][nlon * nlat]. Selection, refusals (per
 * view those of cmi_gpu_set_sky_camera, the message names the view) and
 * CMI_GPU_ENOMEM as cmi_gpu_set_ccd_images; like cmi_gpu_set_sky_camera it
 * serves the cell source only. Synchronous. */
int cmi_gpu_set_sky_cameras(cmi_gpu_engine *engine, int32_t nviews,
                            const double *origins, const double *frames,
                            double lon_min, double lon_max, double lat_min,
                            double lat_max, int32_t nlon, int32_t nlat,
                            const double *exclusion_radii,
                            int32_t direct_light);

/* cmi_gpu_download_image for view `view` of the stack (view 0 with a single
 * camera; cmi_gpu_download_image itself returns view 0). A view outside
 * [0, nviews) is CMI_GPU_EINVAL. cmi_gpu_reset_image clears the whole stack
 * and the counters of every view; cmi_gpu_get_dust_counters counts the walk
 * and all views, cmi_gpu_get_sky_camera_counters sums over the views.
 * cmi_gpu_dust_shoot sizes its launches from the steps per packet of the walk
 * and all views, but with several views not below 4 times the lanes the
 * device holds at once (2^19 packets on 256 CUs; 2^20 stays the cap): a
 * smaller launch would leave SIMDs idle without ending sooner. */
int cmi_gpu_download_image_view(cmi_gpu_engine *engine, int32_t view,
                                double *I, double *Q, double *U);

/* counters[4] of view `view` since the last reset = {DDA steps of the view's
 * own marches (the direct light's and the peel-offs'), fp64 atomics into its
 * image, events inside its exclusion radius, events outside its window}; the
 * last two are 0 for parallel views. The steps of cmi_gpu_get_dust_counters
 * are those of the walk (the forced first interaction and the flights
 * between scatterings) plus these over all views. CMI_GPU_ESTATE unless
 * several views are selected. Synchronous. */
int cmi_gpu_get_dust_view_counters(cmi_gpu_engine *engine, int32_t view,
                                   uint64_t *counters);

/* The view that the camera-dependent probes of cmi_gpu_dust_probe (4 TRACE,
 * 6 SKY_PEEL) follow: they run the single camera's probe for that view, so a
 * row is exactly the single camera's row. View 0 after every call that sets
 * a camera. */
int cmi_gpu_select_probe_view(cmi_gpu_engine *engine, int32_t view);

/* ------------------------------------------------ emission-line images -- */
/* Ray-traced line-of-sight maps of the grid: what an observer in the
 * direction (theta, phi) sees of the cells' emissivities, with dust
 * extinction along the ray. The reference has no such mode (its users sum
 * cells along an axis in Python; SurfaceDensityCalculator does it for
 * densities along z). The geometry is that of the CCD image above
 * (src/CCDImage.hpp:242-270), inverted:
 *   n   = (sin theta cos phi, sin theta sin phi, cos theta)   to the observer
 *   e_x = (-sin phi, cos phi, 0),  e_y = (-cos theta cos phi,
 *         -cos theta sin phi, sin theta)
 * a world point p projects to (p . e_x, p . e_y); pixel (ix, iy) is stored
 * at ix * ny + iy. With supersampling s, sample (a, b) of a pixel has image
 * coordinates anchor + sides * ((ix + (a + 0.5) / s) / nx, (iy + (b + 0.5) /
 * s) / ny); its ray x e_x + y e_y + t n runs through the box from the far
 * side to the observer's (a slab test; a ray that misses contributes 0) and
 * is marched cell by cell with the exact marcher's arithmetic. Per cell with
 * extinction coefficient k (m^-1), emissivity j (J m^-3 s^-1) and path ds:
 *   k == 0:  I += (j / 4 pi) ds
 *   else:    dtau = k ds,  I = I exp(-dtau) + (j / 4 pi / k) (-expm1(-dtau))
 * A pixel is the mean of its s^2 samples (summed a outer, b inner): surface
 * brightness in W m^-2 sr^-1, not normalised. No atomics: the same call on
 * the same state gives the same bits. Periodic boxes are refused
 * (CMI_GPU_EINVAL), blocks of a decomposed grid too (CMI_GPU_ESTATE): an
 * image of one block is not an image. CMI_GPU_EINVAL for nx, ny <= 0,
 * nx ny > 2^28, supersample outside 1..8 (or more than 2^30 samples along
 * an axis), non-positive sides. All three
 * calls are synchronous. */

/* images[k * nx * ny + pixel] (host) of the emission lines lines[k], numbered
 * as in cmi_gpu_compute_emissivities and with its preconditions: it needs
 * the abundances and the state of all 14 ions to mean anything but, like that
 * call, checks only that cell data was set (CMI_GPU_ESTATE). k = n_H
 * dust_cross_section, a cross section per hydrogen nucleus in m^2 (0: no
 * dust; negative: EINVAL). The emissivities are computed on the device, 7
 * lines per march. */
int cmi_gpu_render_line_images(cmi_gpu_engine *engine, int32_t nlines,
                               const int32_t *lines, double theta, double phi,
                               int32_t nx, int32_t ny, const double *anchor,
                               const double *sides, int32_t supersample,
                               double dust_cross_section, double *images);

/* the same for any per-cell quantities: fields[nfields][ncell] and the
 * optional extinction[ncell] (m^-1, may be NULL) are host arrays in the
 * engine's cell order, images[k * nx * ny + pixel]. The fields take the place
 * of j, 1 / 4 pi included: 4 pi times the image of a density is its column
 * density along the view (SurfaceDensityCalculator for any view). Needs only
 * cmi_gpu_create. */
int cmi_gpu_render_field_images(cmi_gpu_engine *engine, int32_t nfields,
                                const double *fields, double theta, double phi,
                                int32_t nx, int32_t ny, const double *anchor,
                                const double *sides, int32_t supersample,
                                const double *extinction, double *images);

/* Parity probe of the ray geometry: the rays through the image coordinates
 * xy[n][2]. out[n][3 + 2 max_cells], fp64: {t_in, t_out, steps, the first
 * max_cells cells, their path lengths}; steps = 0 and t_in = t_out = NaN for
 * a ray that misses the box. n <= 2^24; a coordinate that is not finite is
 * CMI_GPU_EINVAL. */
int cmi_gpu_line_image_probe(cmi_gpu_engine *engine, double theta, double phi,
                             int64_t n, const double *xy, int32_t max_cells,
                             double *out);

/* ------------------------------------------------ spectral line cubes -- */
/* The images of cmi_gpu_render_line_images / cmi_gpu_render_field_images
 * resolved in radial velocity: an image per velocity channel. Geometry, the
 * sample grid, supersampling, the slab test, the march order (far side to
 * observer) and the cell and path-length arithmetic are the images',
 * unchanged. The extinction stays grey dust: no line opacity. Parallel camera
 * only (the camera inside the model: "sky cubes" below).
 *
 * Velocity axis: nchan >= 1 channels of equal width cover the radial
 * velocities [vmin, vmax) in m s^-1, vmax > vmin, both finite; edge
 *   e_c = vmin + c * dv   for c = 0 .. nchan,   dv = (vmax - vmin) / nchan,
 * computed in exactly this form. Radial velocity is positive for matter that
 * recedes from the observer: with n the unit vector to the observer a cell of
 * velocity v has u = -((v_x n_x + v_y n_y) + v_z n_z).
 *
 * Line profile: a cell has the Gaussian width b = sqrt(2) sigma, sigma^2 =
 * k_B T / (A m_u) + sigma_turb^2 (computed as b = sqrt(2 (k_B T / (A m_u) +
 * sigma_turb sigma_turb)), k_B = 1.38064852e-23 J K^-1, m_u = 1.660539040e-27
 * kg), A the standard atomic weight of the emitting element:
 *   H 1.00794  He 4.002602  C 12.0107  N 14.0067  O 15.9994  Ne 20.1797
 *   S 32.065
 * A blended entry (OII_3727, SII_6725, ...) is one line at one rest velocity.
 * The fraction of a cell's emission in channel c is
 *   f_c = 0.5 * (E((e_{c+1} - u) / b) - E((e_c - u) / b)),
 *   E(z) = 1 for z >= 6, -1 for z <= -6, erf(z) otherwise
 * (fp64 erf is exactly 1 from |z| = 5.95 on: the clamp is no approximation).
 * For b == 0 E is the step function with the lower edge inclusive: E = 1 for
 * e > u and -1 for e <= u, all emission goes to the channel with e_c <= u <
 * e_{c+1}, and no NaN arises.
 *
 * Per step of length ds in a cell with the images' record {k, s} (s = j / 4
 * pi, or j / 4 pi / k where k != 0), the product in parentheses first:
 *   k == 0:  I_c += (s ds) f_c
 *   else:    dtau = k ds,  I_c = I_c exp(-dtau) + (s * -expm1(-dtau)) f_c
 *
 * Output: channel-integrated surface brightness, W m^-2 sr^-1 per channel
 * (not per m s^-1: dividing by dv is the caller's), cube[(l * nchan + c) * nx
 * * ny + ix * ny + iy]; a pixel is the mean of its s^2 samples, summed a
 * outer, b inner. No atomics: the same call gives the same bits.
 *
 * What follows from these definitions: (1) with nchan = 1, vmin <= u - 6 b
 * and vmax >= u + 6 b for every cell, f_0 = 1 exactly and the cube is the
 * image of the same view, bit for bit; (2) adding one constant to every u,
 * vmin and vmax leaves the cube unchanged (bit for bit where every e - u
 * stays exact); (3) the sum over channels is at most the image, and equal to
 * it up to rounding when the range covers u +- 6 b of every emitting cell.
 *
 * Preconditions and errors of the image calls; also CMI_GPU_EINVAL for nchan
 * < 1, vmax <= vmin or a range that is not finite, and for nlines * nchan *
 * nx * ny > 2^28. All calls are synchronous; a call that fails leaves the
 * engine usable. */

/* A of the element that emits emission line `line` (numbered as in
 * cmi_gpu_compute_emissivities); 0 for an entry that has no cube, and for a
 * number that is no entry. Host only, no engine. */
double cmi_gpu_emission_line_atomic_weight(int32_t line);

/* The bulk velocities of the cells, v[3][ncell] (host, m s^-1, the engine's
 * cell order), for cmi_gpu_render_line_cube. NULL drops the array: every cell
 * is then at rest, as before the first call. A component that is not finite
 * is CMI_GPU_EINVAL (checked on the device) and the previous state is kept. */
int cmi_gpu_set_cell_velocities(cmi_gpu_engine *engine,
                                const double *velocities);

/* cube (host) of the emission lines lines[l]: lines, dust_cross_section and
 * preconditions as in cmi_gpu_render_line_images, velocities from
 * cmi_gpu_set_cell_velocities, widths from the cells' temperatures and
 * sigma_turb (m s^-1; negative or NaN: EINVAL). Entries that are not the
 * line of one ion (HII, BALMER_JUMP_*, avg_*, Hrec_s, WFC2_*) are
 * CMI_GPU_EINVAL. The emissivities are computed once per batch of 7 lines,
 * not per channel. */
int cmi_gpu_render_line_cube(cmi_gpu_engine *engine, int32_t nlines,
                             const int32_t *lines, double theta, double phi,
                             int32_t nx, int32_t ny, const double *anchor,
                             const double *sides, int32_t supersample,
                             double dust_cross_section, int32_t nchan,
                             double vmin, double vmax, double sigma_turb,
                             double *cube);

/* the same for any per-cell sources: fields[nfields][ncell] and the optional
 * extinction[ncell] as in cmi_gpu_render_field_images, velocity[3][ncell]
 * (m s^-1; NULL: at rest; not finite: EINVAL) and widths[nfields][ncell] (b
 * in m s^-1, >= 0 and finite, else EINVAL). Needs only cmi_gpu_create. */
int cmi_gpu_render_field_cube(cmi_gpu_engine *engine, int32_t nfields,
                              const double *fields, const double *extinction,
                              const double *velocity, const double *widths,
                              double theta, double phi, int32_t nx, int32_t ny,
                              const double *anchor, const double *sides,
                              int32_t supersample, int32_t nchan, double vmin,
                              double vmax, double *cube);

/* ------------------------------------------------------------ sky maps -- */
/* Line images for an observer inside or near the grid: the other camera. The
 * calls above see the box from infinitely far away, one direction for all
 * rays; here a call has one origin o (metres, any finite point, inside or
 * outside the box) and nrays directions d_r, and ray r is o + t d_r, t >= 0:
 * an all-sky map from a point of the model, or pencil beams towards catalogue
 * positions. The reference has no such mode.
 *
 * The directions are used exactly as given and are not normalised on the
 * device. The host refuses the call (CMI_GPU_EINVAL, nothing is launched) if
 * an origin or direction component is not finite or if |d|^2 differs from 1
 * by more than 1e-9. Components that are exactly zero are allowed (they take
 * the DBL_MAX branch of the step).
 *   Slab test: that of the images above with the ray's own 1 / d per axis:
 *     t0 = (lo - o) (1 / d), t1 = (hi - o) (1 / d), t_in = max over axes of
 *     min(t0, t1), t_out = min of max(t0, t1); an axis with d == 0 only asks
 *     lo <= o < hi.
 *   Hit: t_start = max(t_in, 0); the ray hits if t_start < t_out and t_out is
 *     finite. A ray that misses gives 0.
 *   Start: with the origin in the box (t_in <= 0) at o itself, otherwise at
 *     o + t_in d; in the cell floor((p - anchor) inv_cellside) gives, clamped
 *     into the grid. An origin exactly on a cell wall with a direction
 *     pointing back across that wall makes a first step of length 0: allowed,
 *     not special-cased (an origin on a box face pointing outwards misses).
 *   Step: the exact marcher's (dda_step<false> at tau = HUGE_VAL), as in the
 *     images above: walls from the index, every axis that ties the minimum
 *     advances. The march ends when the index leaves the grid.
 *   Integration, from the observer outwards, with transmission T = 1 and
 *     I_l = 0 at the start; a cell {k, s_l} (s = j / 4 pi, or j / 4 pi / k
 *     where k != 0) with path ds does
 *       k == 0:  I_l += T * (s_l * ds)
 *       else:    dtau = k * ds;  I_l += T * (s_l * (-expm1(-dtau)));
 *                T = T * exp(-dtau)
 *     in exactly this order of multiplications.
 * Results are surface brightnesses in W m^-2 sr^-1, the unit of the images
 * above. One lane per ray in the caller's order (wave w takes rays 64 w ..
 * 64 w + 63), at most 2^22 rays per launch, 7 sources per march. No atomics:
 * the same call on the same state gives the same bits. Periodic boxes are
 * refused (CMI_GPU_EINVAL), blocks of a decomposed grid too (CMI_GPU_ESTATE).
 * All calls are synchronous; a call that fails leaves the engine usable. */

/* out[k * nrays + r] (host) of the emission lines lines[k] along ray r;
 * lines, dust_cross_section and preconditions as in
 * cmi_gpu_render_line_images. 1 <= nrays <= 2^28. */
int cmi_gpu_render_line_sky(cmi_gpu_engine *engine, int32_t nlines,
                            const int32_t *lines, const double origin[3],
                            int64_t nrays,
                            const double *directions /* [nrays][3] */,
                            double dust_cross_section,
                            double *out /* [nlines][nrays] */);

/* the same for any per-cell quantities, fields and extinction as in
 * cmi_gpu_render_field_images */
int cmi_gpu_render_field_sky(cmi_gpu_engine *engine, int32_t nfields,
                             const double *fields, const double origin[3],
                             int64_t nrays, const double *directions,
                             const double *extinction,
                             double *out /* [nfields][nrays] */);

/* Parity probe of the ray geometry: out[n][3 + 2 max_cells], fp64: {t_start,
 * t_out, steps, the first max_cells cells, their path lengths}; steps = 0 and
 * t_start = t_out = NaN for a ray that misses. 1 <= n <= 2^24. */
int cmi_gpu_sky_probe(cmi_gpu_engine *engine, const double origin[3],
                      int64_t n, const double *directions, int32_t max_cells,
                      double *out);

/* An equirectangular map, host code over cmi_gpu_render_line_sky: pixel
 * (i, j), i < nlon, j < nlat, is stored at i * nlat + j; its centre is
 *   l = lon_min + (lon_max - lon_min) (i + 0.5) / nlon,  b likewise,
 * its direction d = cos b cos l e_1 + cos b sin l e_2 + sin b e_3 with e_1,
 * e_2, e_3 the rows of frame[9], which must be orthonormal to 1e-9 (every
 * |e_i . e_j - delta_ij| <= 1e-9; CMI_GPU_EINVAL otherwise; the directions
 * then pass the ray-list call's own check like any caller's). Radians;
 * lon_min < lon_max, -pi / 2 <= lat_min < lat_max <= pi / 2, nlon nlat <=
 * 2^28. The rays are marched in 8 x 8 tiles of the map and the results put
 * back in pixel order on the host; the values do not depend on that order.
 * maps[k * nlon * nlat + pixel]. */
int cmi_gpu_render_line_sky_map(cmi_gpu_engine *engine, int32_t nlines,
                                const int32_t *lines, const double origin[3],
                                const double frame[9], double lon_min,
                                double lon_max, double lat_min, double lat_max,
                                int32_t nlon, int32_t nlat,
                                double dust_cross_section, double *maps);

/* The map's directions[nlon * nlat][3] in pixel order, by the function the
 * map call uses (host only, no engine), and the exact solid angles of the
 * pixels, dl (sin b_hi - sin b_lo), so that a flux is sum(I omega). Either
 * output may be NULL. */
int cmi_gpu_sky_map_directions(const double frame[9], double lon_min,
                               double lon_max, double lat_min, double lat_max,
                               int32_t nlon, int32_t nlat, double *directions,
                               double *solid_angles);

/* ----------------------------------------------------------- sky cubes -- */
/* The sky maps above resolved in radial velocity: a sky value per velocity
 * channel, for an observer inside or near the grid - the longitude-latitude-
 * velocity cube such an observer records, or a spectrum per pencil beam.
 *
 * Rays: the ray list o + t d_r, the origin, the checks of the directions, the
 * slab test, the start cell, the step and the end of the march are those of
 * "sky maps", unchanged, and so are the refusals of periodic boxes
 * (CMI_GPU_EINVAL) and of blocks of a decomposed grid (CMI_GPU_ESTATE).
 *
 * Velocity axis: the edges e_c = vmin + c * dv, E(z) and f_c are those of
 * "spectral line cubes", unchanged, b == 0 as the step function with the
 * lower edge inclusive included, and so are the atomic weights and b =
 * sqrt(2 (k_B T / (A m_u) + sigma_turb sigma_turb)).
 *
 * Radial velocity: this is what is new. A cell of velocity v seen by an
 * observer of velocity v_obs along the ray direction d (which points away
 * from the observer) has
 *   w = v - v_obs   per component, formed once per cell,
 *   u = (w_x d_x + w_y d_y) + w_z d_z
 * in exactly this form, no contraction. u is positive for matter that
 * recedes. There is no minus sign: d points away from the observer, where the
 * parallel camera's n points towards it.
 *
 * Per step of length ds, from the observer outwards, T = 1 and I_c = 0 at the
 * start, with the sky march's own products:
 *   k == 0:  I_c += T * ((s * ds) * f_c)
 *   else:    dtau = k * ds;  I_c += T * ((s * -expm1(-dtau)) * f_c);
 *            T = T * exp(-dtau)
 * in this order of multiplications.
 *
 * Output: channel-integrated surface brightness, W m^-2 sr^-1 per channel,
 * out[(l * nchan + c) * nrays + r]. No atomics: the same call on the same
 * state gives the same bits.
 *
 * What follows: (1) with nchan = 1 and a range that covers u +- 6 b of every
 * cell on every ray the result is that of cmi_gpu_render_field_sky /
 * cmi_gpu_render_line_sky, bit for bit; (2) adding one vector to every cell's
 * velocity and to v_obs changes nothing, bit for bit where the subtractions
 * are exact; (3) the channels sum to at most the sky value, and to it up to
 * rounding when the range covers everything; (4) the map call equals the
 * ray-list call on the map's directions, bit for bit.
 *
 * Errors: those of the sky calls and of the cube calls; also CMI_GPU_EINVAL
 * for an observer velocity that is not finite and for nlines * nchan * nrays
 * > 2^28. observer_velocity may be NULL (at rest). All calls are synchronous;
 * a call that fails leaves the engine usable and the state of
 * cmi_gpu_set_cell_velocities untouched. 6 sources per march. */

/* fields, extinction and origin / rays as in cmi_gpu_render_field_sky,
 * velocity and widths as in cmi_gpu_render_field_cube. Needs only
 * cmi_gpu_create. */
int cmi_gpu_render_field_sky_cube(cmi_gpu_engine *engine, int32_t nfields,
                                  const double *fields,
                                  const double *extinction,
                                  const double *velocity /* [3][ncell] or NULL */,
                                  const double *widths, const double origin[3],
                                  const double *observer_velocity /* [3] or NULL */,
                                  int64_t nrays, const double *directions,
                                  int32_t nchan, double vmin, double vmax,
                                  double *out /* [nfields][nchan][nrays] */);

/* lines, rays and dust_cross_section as in cmi_gpu_render_line_sky; the
 * velocities come from cmi_gpu_set_cell_velocities, the widths from the
 * cells' temperatures and sigma_turb as in cmi_gpu_render_line_cube. Entries
 * that are not the line of one ion are CMI_GPU_EINVAL. */
int cmi_gpu_render_line_sky_cube(cmi_gpu_engine *engine, int32_t nlines,
                                 const int32_t *lines, const double origin[3],
                                 const double *observer_velocity,
                                 int64_t nrays, const double *directions,
                                 double dust_cross_section, int32_t nchan,
                                 double vmin, double vmax, double sigma_turb,
                                 double *out /* [nlines][nchan][nrays] */);

/* The map of cmi_gpu_render_line_sky_map per channel: host code over
 * cmi_gpu_render_line_sky_cube with the map's 8 x 8 tile order;
 * cubes[(l * nchan + c) * nlon * nlat + i * nlat + j]. */
int cmi_gpu_render_line_sky_map_cube(cmi_gpu_engine *engine, int32_t nlines,
                                     const int32_t *lines,
                                     const double origin[3],
                                     const double frame[9], double lon_min,
                                     double lon_max, double lat_min,
                                     double lat_max, int32_t nlon,
                                     int32_t nlat, double dust_cross_section,
                                     const double *observer_velocity,
                                     int32_t nchan, double vmin, double vmax,
                                     double sigma_turb, double *cubes);

/* ------------------------------------------ scattered-light line cubes -- */
/* The Monte Carlo images of cmi_gpu_dust_shoot resolved in radial velocity:
 * the line profile of the direct and the dust-scattered light per pixel, for
 * the cell source and any of the cameras above (parallel or point, one view or
 * several). No counterpart in the reference.
 *
 * Grey dust makes the walk independent of frequency: cube mode draws no
 * random number, a cube run walks the image run's walk, and its image is the
 * image run's image but for the order of the atomics.
 *
 * Conventions. Channels, the edges e_c = vmin + c * dv, E(z), f_c, the case
 * b == 0 and "positive = receding" are exactly those of "spectral line cubes"
 * above. dot3(a, b) = (a_x b_x + a_y b_y) + a_z b_z in this order, no
 * contraction. v_c is the bulk velocity of cell c from
 * cmi_gpu_set_cell_velocities, zero for every cell when none was set; sigma_t
 * the turbulent dispersion; s2_c a per-cell variance built when cube mode is
 * set:
 *   line source:  s2_c = k_B T_c / (A m_u) + sigma_t * sigma_t, with the
 *                 constants and atomic weights of "spectral line cubes";
 *   field source: s2_c = 0.5 * b_c * b_c from the caller's widths[ncell].
 *
 * A packet carries two more scalars: q, its Doppler velocity (positive =
 * blue-shifted in the lab frame), and s2, the variance of its profile.
 *   Emission in cell e along k:  q = dot3(v_e, k);  s2 = s2_e.
 *   Direct light from e towards the observer along d (the parallel camera's
 *   direction to the observer; for the point camera the unit vector k = v / r
 *   from the event to the observer):
 *     parallel:  u = -dot3(v_e, d)   (the u of "spectral line cubes", bit for
 *                bit);
 *     point:     u = -(dot3(v_e, d) - dot3(v_obs, d));
 *     b = sqrt(2 * s2_e).
 *   Peel-off at a scattering in cell s, incoming direction k, towards d:
 *     u = -((q + (dot3(v_s, d) - dot3(v_s, k))) - dot3(v_obs, d)), the v_obs
 *     term absent for the parallel camera;
 *     b = sqrt(2 * (s2 + (2 * sigma_t * sigma_t) * fmax(0, 1 - dot3(k, d)))).
 *   Flying on after the scattering gave k':
 *     q += dot3(v_s, k') - dot3(v_s, k);
 *     s2 += (2 * sigma_t * sigma_t) * fmax(0, 1 - dot3(k, k')).
 * The emission cell e is the cell the source selected. The scattering cell s
 * is floor((pos - anchor) * inv_cellside) per axis, clamped into the grid -
 * not whatever index a march ended with.
 *
 * Dust that shares the gas's turbulence: the scattering grain moves with the
 * bulk velocity of its cell plus a turbulent velocity of dispersion sigma_t
 * per component. A grain of velocity w shifts the light it redirects from k
 * to k' by w . (k' - k); over the turbulent part that is a Gaussian of
 * variance sigma_t^2 |k' - k|^2 = 2 sigma_t^2 (1 - k . k'), which is what
 * s2 grows by per scattering. With sigma_t = 0 the profile keeps the
 * emitting cell's thermal width.
 *
 * Deposit. An event that adds (wI, wQ, wU) to a pixel of the image also adds
 * (wI f_c, wQ f_c, wU f_c) to channel c of that pixel's spectrum, for every c
 * with f_c != 0; zero addends cost no atomic. Every cube atomic is counted in
 * natomics (and in the view's). The image is filled as before in the same
 * run. Events that add nothing to the image (outside the window, inside the
 * exclusion radius, missed pixels) add nothing to the cube and are counted as
 * before.
 *
 * What follows: (1) one channel that covers every u +- 6 b has f_0 = 1
 * exactly, and the cube is the image of the same run up to the order of the
 * atomics; (2) the channels of a covering cube sum to the image up to
 * rounding; (3) adding one vector V to every cell velocity changes every u by
 * -dot3(V, d) and nothing else (the sum over scatterings telescopes): for the
 * parallel camera shifting vmin and vmax by that amount gives the same cube
 * up to rounding, for the point camera adding V to the observer's velocity
 * as well changes nothing; (4) with all cells at rest, sigma_t = 0 and one
 * temperature the cube is the image times the constant f_c(0, b); (5) at
 * albedo 0 the cube converges to the ray-traced cube of
 * cmi_gpu_render_line_cube / cmi_gpu_render_line_sky_map_cube in the unit of
 * the scattered-light images' scaling. */

/* Switches cube mode on for the cameras as currently set: allocates and
 * zeroes the cubes, builds s2, and resets the image and the counters.
 * observer_velocities is [nviews][3] (m s^-1; the point cameras', ignored by
 * parallel ones) or NULL (at rest). nchan = 0 switches cube mode off and
 * frees the buffers (the other arguments are then not looked at).
 * CMI_GPU_ESTATE: no camera; no cell source selected (the spiral galaxy has
 * no line) or a stale one; widths given with a line source, or missing with a
 * field source. CMI_GPU_EINVAL: the line source's entry is not the line of
 * one ion; nchan < 0, a range that is not finite with vmax > vmin; a
 * sigma_turb that is negative or not finite; a width that is negative or not
 * finite; an observer velocity that is not finite; nviews * nchan * npixel >
 * 2^28. CMI_GPU_ENOMEM if the cubes do not fit. A call that fails leaves the
 * previous state in place.
 * Cube mode is stale, and the next shoot or probe fails with CMI_GPU_ESTATE
 * until this call is made again, once the cell source is stale or set again,
 * a camera is set again, or the velocities are replaced. Synchronous. */
int cmi_gpu_set_scattered_cube(cmi_gpu_engine *engine, int32_t nchan,
                               double vmin, double vmax, double sigma_turb,
                               const double *widths /* [ncell] or NULL */,
                               const double *observer_velocities
                               /* [nviews][3] or NULL */);

/* The cube of view `view` (0 with a single camera), unnormalised: I, Q, U
 * host [nchan][npixel] each, in the pixel order of the view's image; any of
 * the three may be NULL. Fails where cmi_gpu_download_image_view fails, and
 * with CMI_GPU_ESTATE if cube mode is off or stale. cmi_gpu_reset_image also
 * zeroes the cubes. With cube mode on cmi_gpu_dust_shoot launches the cube
 * kernels (same signature, same launch sizing), and cmi_gpu_dust_probe has
 *  7 CUBE_TRACE: 4 TRACE with rows of 10 doubles, the 8 of TRACE and then
 *    {u, b} of the event (0, 0 for an event inside the exclusion radius);
 *    CMI_GPU_ESTATE unless cube mode is on.
 * Synchronous. */
int cmi_gpu_download_cube_view(cmi_gpu_engine *engine, int32_t view, double *I,
                               double *Q, double *U);

/* -------------------------------------------------------- Lyman alpha -- */
/* Monte Carlo transfer of the Lyman-alpha line: packets from the cell source
 * scatter resonantly off H I and off dust, are redistributed in frequency at
 * every hydrogen scattering, and are peeled off towards the parallel cameras
 * into an image and a velocity cube per view (Stokes I). No counterpart in
 * the reference. tests/support/lyman_alpha_reference.c restates everything
 * below in plain C, random number for random number.
 *
 * Constants: lambda_0 = 1215.67e-10 m, A_21 = 6.265e8 s^-1, h nu_0 = h c /
 * lambda_0 with the engine's h and c; m_H = 1.00794 m_u, the mass "spectral
 * line cubes" uses for H alpha's width. dot3(a, b) = (a_x b_x + a_y b_y) +
 * a_z b_z, no contraction.
 *
 * Per cell, built into one 64-byte record {kappa_0, 1 / b, a, kappa_d, v_x,
 * v_y, v_z, n_HI} when the mode is set:
 *   b       = sqrt(2 * (k_B T / m_H + sigma_t * sigma_t))
 *   a       = A_21 * lambda_0 / (4 * pi * b)
 *   kappa_0 = n_HI * (3 lambda_0^3 A_21 / (8 pi sqrt(pi))) / b  (5.90e-14 cm^2
 *             per atom at 1e4 K); n_HI = n_H x_H of the cells, or the caller's
 *   kappa_d = n_H sigma_d, sigma_d the cross section per hydrogen nucleus of
 *             cmi_gpu_set_dust_scattering_per_hydrogen; 0 if no dust is set
 *   v       = the cell's velocity (cmi_gpu_set_cell_velocities), 0 if none.
 *
 * A packet carries its lab-frame shift as a velocity q (positive = blue). In
 * a cell, flying along k: x = (q - dot3(v, k)) * (1 / b), kappa(x) = kappa_0
 * H(a, x) + kappa_d, with z = (x^2 - 0.855) / (x^2 + 3.42) and
 *   H(a, x) = sqrt(pi) * Q + E,
 *   Q = 0 for z <= 0, else (1 + 21 / x^2) * a / (pi * (x^2 + 1)) * (z * (0.1117
 *       + z * (4.421 + z * (-9.207 + 5.674 * z)))),
 *   E = exp(-x^2) for x^2 < 64, else 0
 * (within 2.2 % of the Voigt function for |x| <= 1000 between 10 K and 1e5 K).
 *
 * Random numbers of packet i (stream seed, iteration 0, packet i):
 *   6   the cell source's draws (cell, position, direction), as dust_shoot's
 *   4   the emitting atom: r_1 = sqrt(-ln R), f_1 = 2 pi R', r_2, f_2 likewise;
 *       w_e = v + b * (r_1 cos f_1, r_1 sin f_1, r_2 cos f_2);  q = dot3(w_e, k)
 *   1   the forced first optical depth -ln(1 - R (1 - exp(-tau_max))), tau_max
 *       the depth to the box edge along k at q
 *   then per event, at the position the walk stopped, in the cell floor((pos -
 *   anchor) * inv_cellside) clamped into the grid:
 *   1   the species: hydrogen if R < kappa_0 H / kappa of that cell
 *   hydrogen:
 *   3n  u_par from f(u) ~ exp(-u^2) / ((x - u)^2 + a^2) by the rejection method
 *       of Zheng & Miralda-Escude (2002) for |x|, the sign restored afterwards:
 *       e_0 = exp(-u_0^2), th_0 = atan((u_0 - |x|) / a), p = (th_0 + pi / 2) /
 *       ((1 - e_0) th_0 + (1 + e_0) pi / 2); per attempt {R_1, R_2, R_3}: R_1 <=
 *       p: th = -pi / 2 + R_2 (th_0 + pi / 2), u = a tan(th) + |x|, accepted if
 *       R_3 <= exp(-u^2); else th = th_0 + R_2 (pi / 2 - th_0), accepted if R_3
 *       <= exp(-u^2) / e_0. The separation point is that of Laursen et al.
 *       (2009) up to their core-wing transition: u_0 = 0 for |x| < 0.2, max(0,
 *       |x| - 0.01 a^(1/6) exp(1.2 |x|)) for |x| < x_cw = 1.59 - 0.60 log10 a -
 *       0.03 log10^2 a, else min(4, max(0, |x| - 0.5)); it changes the
 *       acceptance rate only (at least 0.046 for |x| <= 12, about 1.8 / |x|
 *       far in the wing). After 1e6 rejections the last candidate is taken.
 *   2   rho = sqrt(s - ln R) with s = x_crit^2 if |x| < x_crit, else 0; psi =
 *       2 pi R'; u_1 = rho cos psi, u_2 = rho sin psi
 *       w = v + b * ((u_par k + u_1 e_1) + u_2 e_2) per component, e_1 = (cos
 *       theta cos phi, cos theta sin phi, -sin theta), e_2 = (-sin phi, cos
 *       phi, 0) from the angles of k
 *   2   the new isotropic direction k' {cos theta, phi}; q += dot3(w, k') -
 *       dot3(w, k); Q = U = V = 0
 *   dust: the albedo multiplies the weight; DustScattering's scatter draws k'
 *       (1 or 2 uniforms) and changes the Stokes vector as in dust_shoot; the
 *       grain has the cell's velocity: q += dot3(v, k') - dot3(v, k)
 *   1   the next optical depth -ln R.
 * A packet that has scattered max_scatter times is stopped and counted.
 *
 * Events (per view, direction d to the observer): q_d = dot3(w_e, d) for the
 * direct light, q + (dot3(w, d) - dot3(w, k)) for a peel-off (w the atom's
 * velocity, or the cell's for dust); tau the depth to the box edge along d at
 * q_d; the addend ((W * P) * exp(-tau)) * I with W = 1 for the direct light
 * and forced weight * albedos otherwise, P = 0.25 / pi for hydrogen and the
 * direct light (isotropic) and DustScattering's scatter_towards for dust, I
 * the packet's Stokes I (after scatter_towards for dust). It goes into the
 * pixel of the event's position and into the channel c with e_c <= u <
 * e_{c+1}, u = -q_d, e_c = vmin + c * dv (a delta in velocity; the lower edge
 * inclusive, as for b == 0 in "spectral line cubes"). An event outside
 * [vmin, vmax) goes into the image only.
 *
 * What follows: a cube that covers every u sums to the image; with n_HI = 0
 * and no dust only the direct light remains, a thin Gaussian line of width b;
 * adding V to every velocity shifts every u by -dot3(V, d).
 *
 * Not modelled: recoil, deuterium, fine structure, the dipole phase function
 * and the line's own polarisation, collisional excitation, an adaptive core
 * skipping. */

/* Switches the mode on for the parallel camera(s) as currently set: builds
 * the records from the cells (n_HI and temperature: [ncell] of the caller's,
 * or NULL for n_H x_H and T of the cells), the dust as set and the velocities
 * as set, allocates and zeroes image, cube and counters. x_crit >= 0 is the
 * core-skipping frequency (0: none), max_scatter the cap (1 to 1e8: the
 * stream's block counter has 32 bits). nchan = 0 switches the mode off and
 * frees the buffers. CMI_GPU_ESTATE: a block of a decomposed grid; no cells,
 * no camera, a point camera, no cell source or a stale one; dust that is not
 * per hydrogen nucleus. CMI_GPU_EINVAL: a periodic box; nchan < 0, a range
 * that is not finite with vmax > vmin, sigma_turb or x_crit negative or not
 * finite, max_scatter 0 or above 1e8, a cell whose b is not positive and
 * finite or whose density is negative or not finite, too many values.
 * CMI_GPU_ENOMEM if the cubes do not fit. A call that fails leaves the
 * previous state in place. The mode is stale, and shoot, probe and download
 * fail with CMI_GPU_ESTATE until this call is made again, once a camera, the
 * cell source or the velocities are set again. Synchronous. */
int cmi_gpu_set_lyman_alpha(cmi_gpu_engine *engine, int32_t nchan, double vmin,
                            double vmax, double sigma_turb, double x_crit,
                            uint64_t max_scatter,
                            const double *n_HI /* [ncell] or NULL */,
                            const double *temperature /* [ncell] or NULL */);

/* Packets [first_packet, first_packet + n) of the stream `seed`, added to the
 * image, the cube and the counters; launched in chunks. Asynchronous. */
int cmi_gpu_lya_shoot(cmi_gpu_engine *engine, uint32_t seed,
                      uint64_t first_packet, uint64_t n);

/* Device functions row by row, for parity tests; row k of kind
 *  0 VOIGT: in {a, x, kappa_0, kappa_d}, out {H, kappa_0 * H + kappa_d};
 *  1 OPTICAL_DEPTH: in {pos[3], dir[3], q}, out {tau to the box edge, steps};
 *  2 SAMPLER: in {x, a}, out {u_par, rejections} from the stream of packet
 *    first_packet + k;
 *  3 TRACE: out {events, hydrogen scatterings, dust scatterings, steps, capped,
 *    rejections, rows[max_events][12]} of packet first_packet + k for the
 *    selected view (cmi_gpu_select_probe_view), a row per event being {pos[3],
 *    k[3], q, addend, species (0 direct, 1 hydrogen, 2 dust), u, u_par, x}
 *    with k and q the incoming ones.
 * out is [n][2], or [n][6 + 12 * max_events] for TRACE. Synchronous. */
int cmi_gpu_lya_probe(cmi_gpu_engine *engine, int32_t kind, uint32_t seed,
                      uint64_t first_packet, int64_t n, const double *in,
                      double *out, int32_t max_events);

/* View `view`, unnormalised: image host [nx][ny], cube host [nchan][nx][ny];
 * either may be NULL. CMI_GPU_ESTATE if the mode is off or stale, or a packet
 * reached the cap (the image is incomplete). Synchronous. */
int cmi_gpu_download_lya_view(cmi_gpu_engine *engine, int32_t view,
                              double *image, double *cube);

/* Zeroes image, cube and counters. Synchronous. */
int cmi_gpu_reset_lya(cmi_gpu_engine *engine);

/* {cell crossings, scatterings off hydrogen, off dust, rejections of the atom
 * sampler, atomics, capped packets, packets} since the last reset. */
int cmi_gpu_get_lya_counters(cmi_gpu_engine *engine, uint64_t *counters /*[7]*/);

/* The Lyman-alpha emissivity of the cells as they are, recombinations only, W
 * m^-3 into out[ncell]: f_alpha(T) alpha_B(T) n_e n_p h nu_0, alpha_B =
 * 2.753e-14 L^1.5 / (1 + (L / 2.74)^0.407)^2.242 cm^3 s^-1 with L = 315614 / T
 * (Hui & Gnedin 1997), f_alpha = 0.686 - 0.106 log10(T_4) - 0.009 T_4^-0.44
 * (Cantalupo et al. 2008), n_e = n_H ((1 - x_H0) + A_He (1 - x_He0)) as in
 * cmi_gpu_free_free_coefficients, n_p = n_H (1 - x_H0); 0 where T <= 0. */
int cmi_gpu_lyman_alpha_emissivity(cmi_gpu_engine *engine, double *out);

/* ---------------------------------------- Lyman alpha radiation field -- */
/* What a Lyman-alpha run leaves in the gas, cell by cell: the energy density
 * of the line, the scattering rate per atom (which sets the 21-cm spin
 * temperature where collisions do not: Wouthuysen-Field coupling), and the
 * momentum it deposits (the Lyman-alpha radiation pressure). All are sums over
 * the crossings and events of the walk of "Lyman alpha"; the walk, its random
 * numbers, the image, the cube and the counters are the same with the field on
 * or off. No counterpart in the reference.
 * tests/support/lya_field_reference.c restates everything below in plain C.
 *
 * One row of eight doubles per cell, [ncell][8], 64 bytes and 64-byte aligned:
 *   {L, S_H, S_d, G_x, G_y, G_z, N_H, N_d}.
 * In a cell, for a packet of shift q flying along k: kappa_H = kappa_0 H(a, x),
 * kappa_d as in the record, kappa_p = kappa_H + kappa_d * (1 - omega * g) with
 * the albedo omega and the asymmetry g of the dust as set (the share 1 - omega g
 * of its momentum that a packet leaves with the dust on average; all of it
 * with hydrogen, whose re-emission is isotropic).
 *
 * The first flight - the march from the emission point along k at q that finds
 * tau_max - is tallied as an expected value with weight 1: for the crossing of
 * length ds that begins at the depth tau_in (the sum of ds kappa before it)
 * and has dtau = ds * kappa,
 *   l = (ds * exp(-tau_in)) * E(dtau),  E(t) = -expm1(-t) / t, E(0) = 1
 * is the length that the light still in flight covers in the cell (kappa = 0
 * gives l = ds exactly). L += l, S_H += l kappa_H, S_d += l kappa_d, G += (l
 * kappa_p) k. The forced first walk that follows the same path adds nothing to
 * these five. Why an expected value: the forced walk carries only the share 1 -
 * exp(-tau_max) that interacts, on a path drawn from the truncated exponential;
 * the light that leaves unscattered fills the cells too, and one deterministic
 * sum over the crossings the march makes anyway counts both without a second
 * march and without noise.
 *
 * Every later walk - after an event, with the weight W = forced weight *
 * albedos as it stands after the event - is tallied by its track length: for
 * each crossing, with ds the length actually flown in the cell (the backed-off
 * length in the last one), L += W ds, S_H += W ds kappa_H, S_d += W ds kappa_d,
 * G += (W ds kappa_p) k.
 *
 * Collision estimators: a hydrogen event adds the incoming weight W to N_H of
 * the event's cell, a dust event the weight before the albedo is applied to
 * N_d. In expectation N_H = S_H and N_d = S_d cell by cell, with or without
 * core skipping: the check of the weights and of the first-flight estimator
 * that every run carries.
 *
 * The peel-off marches tally nothing. A capped packet keeps what it tallied;
 * the downloads then refuse, as for the image.
 *
 * Physical units, for a run of N packets from a source of L_total W, s =
 * L_total / N and the cell volume V: the energy density s L / (c V) J m^-3; the
 * scattering rate per atom P_alpha = s S_H / (h nu_0 n_HI V) s^-1; the force
 * density s G / (c V) N m^-3. With core skipping (x_crit > 0) S_H and N_H
 * leave out the skipped scatterings: P_alpha is then too small. L and G are as
 * good as the skipping itself: unbiased while a skipped scattering does not
 * move the packet, which holds in the core proper and not for an x_crit beyond
 * it (the force on a static sphere of 10 K gas, a = 0.015,
 * comes out halved with x_crit = 3). */

/* Switches the radiation field of the Lyman-alpha mode on (enable != 0:
 * allocates the rows if need be and zeroes them) or off (frees them). While it
 * is on, cmi_gpu_lya_shoot launches the kernel instantiation that tallies.
 * CMI_GPU_ESTATE if the Lyman-alpha mode is not set; CMI_GPU_ENOMEM if the rows
 * do not fit. cmi_gpu_set_lyman_alpha, called anew, switches the field off;
 * cmi_gpu_reset_lya zeroes the rows with the image. Synchronous. */
int cmi_gpu_set_lya_field(cmi_gpu_engine *engine, int32_t enable);

/* The raw tallies, rows host [ncell][8]. CMI_GPU_ESTATE if the mode or the
 * field is off, if the mode is stale, or after a capped packet. Synchronous. */
int cmi_gpu_download_lya_field(cmi_gpu_engine *engine,
                               double *rows /* [ncell][8] */);

/* The scattering rate per atom and the 21-cm spin temperature it implies,
 * from the tallies, the records and the cells as they are at the call:
 *   P_alpha = s S_H / (h nu_0 n_HI V), 0 where n_HI = 0; s =
 *             luminosity_per_packet (W), n_HI that of the records
 *   x_alpha = 4 P_alpha T_* / (27 A_10 T_gamma), T_* = h nu_10 / k_B = 0.0682 K
 *             with nu_10 = 1420405751.768 Hz and A_10 = 2.8843e-15 s^-1 of "H I
 *             21-cm cubes", T_gamma = background_temperature
 *   x_c     = (C_10 / A_10) (T_* / T_gamma) with collisions != 0, else 0;
 *             C_10 = n_HI kappa_HH(T) + n_e kappa_eH(T), T the cells'
 *             temperature, n_e = n_H ((1 - x_H0) + A_He (1 - x_He0)) as in
 *             cmi_gpu_free_free_coefficients;
 *             kappa_HH = 3.1e-11 T^0.357 exp(-32 / T) cm^3 s^-1 (Kuhlen, Madau
 *             & Montgomery 2006, ApJ 637, L1);
 *             log10(kappa_eH / cm^3 s^-1) = -9.607 + 0.5 log10 T exp(-(log10
 *             T)^4.5 / 1800) for 1 K <= T <= 1e4 K, held at its 1e4 K value
 *             above and at its 1 K value below (Liszt 2001, A&A 371, 698)
 *   T_s     = (1 + x) / (1 / T_gamma + x / T_k), x = x_alpha + x_c, which is
 *             1 / T_s = (1 / T_gamma + x / T_k) / (1 + x): the colour
 *             temperature of the Lyman-alpha field is taken as the kinetic
 *             temperature T_k = T (true after the ~1e3 scatterings that bring
 *             the spectrum near line centre into equilibrium with the gas;
 *             Field 1959). A cell with T_k <= 0 gets T_s = T_gamma.
 * P_alpha host [ncell] or NULL, T_s host [ncell], the argument
 * spin_temperature of cmi_gpu_render_hi_cube and its sky variants with
 * spin_mode 2. CMI_GPU_EINVAL for a scale or a background that is not positive
 * and finite. CMI_GPU_ESTATE as for the download, and if the mode was set with
 * x_crit > 0: the skipped core scatterings would make P_alpha too small, and
 * it is not handed out silently. Synchronous. */
int cmi_gpu_lya_spin_temperature(cmi_gpu_engine *engine,
                                 double luminosity_per_packet,
                                 double background_temperature,
                                 int32_t collisions,
                                 double *P_alpha /* [ncell] or NULL */,
                                 double *T_s /* [ncell] */);

/* --------------------------------------------------- continuum images -- */
/* The formal solution of the transfer equation with an absorption coefficient
 * and a source function of their own in every channel, and thermal free-free
 * emission of the ionized gas as its first client: radio continuum images of
 * an H II region, optically thin at high frequency and with T_b = T_e below
 * the turnover. Every product above shares one grey exp(-k ds) among its
 * channels and emits what the cell does not absorb itself; here the cell
 * absorbs its own emission. No counterpart in the reference.
 *
 * Channels: nf >= 1, in the caller's order. Channel f has a per-cell
 * absorption coefficient kappa_f (m^-1, finite, >= 0), a per-cell source
 * function S_f (W m^-2 Hz^-1 sr^-1, finite) and a background intensity bg_f
 * (finite; background == NULL means all zero).
 *
 * Arithmetic: every product and sum below is one IEEE operation
 * (-ffp-contract=off) in the order written, with one expm1 per cell and
 * channel and no exp.
 *
 * Parallel camera: the view, the sample grid, the supersampling and the
 * average of the samples into pixels are those of cmi_gpu_render_field_images
 * ("emission-line images"), unchanged. The march runs from the far side to
 * the near side. I_f starts at bg_f; per cell with path ds
 *   em = expm1(-(kappa_f * ds));  I_f = I_f + em * (I_f - S_f)
 * A ray that misses the box returns bg_f. Two consequences are exact:
 * kappa == 0 leaves I_f untouched, and I_f == S_f stays S_f - a medium in
 * equilibrium with its background is invisible, bit for bit.
 *
 * Rays from a point: the origin, the direction list and their checks, the
 * slab test, the start cell and the step are those of cmi_gpu_render_field_sky
 * ("sky maps"), unchanged. The march runs from the observer outwards. T_f = 1
 * and I_f = 0 at the start; per cell
 *   em = expm1(-(kappa_f * ds));  I_f = I_f + T_f * (S_f * -em);
 *   T_f = T_f + T_f * em
 * and after the last cell, or for a ray that misses, I_f = I_f + T_f * bg_f.
 *
 * Free-free coefficients of the cells as they are, with the constants h, k_B
 * and c of the engine (CODATA 2014: 6.626070040e-34, 1.38064852e-23,
 * 299792458):
 *   n_e = n * ((1 - x_H0) + A_He * (1 - x_He0)),  n_i = n_e
 *     (A_He from cmi_gpu_set_abundances; both ions have charge 1),
 *   x   = (h * nu) / (k_B * T),
 *   S   = (2 * h * nu * nu * nu / (c * c)) / expm1(x)           = B_nu(T),
 *   g   = log(exp(5.960 - (sqrt(3) / pi) * log((nu / 1e9) * pow(T / 1e4,
 *         -1.5))) + e)                        (Draine 2011, eq. 10.9),
 *   j   = 5.444364709e-52 * g * n_e * n_i / sqrt(T) * exp(-x)
 *         (W m^-3 Hz^-1 sr^-1; the Gaussian (2^5 pi e^6 / (3 m_e c^3))
 *         sqrt(2 pi / (3 k_B m_e)) / (4 pi) times 1e-13 for SI densities),
 *   kappa = j / S                                      (Kirchhoff's law),
 * the products from left to right. A cell with n_e == 0, without a positive
 * temperature or with S == 0 has kappa = 0 and S = 0 exactly: vacuum and
 * neutral cells give no NaN.
 *
 * Frequencies: finite and > 0 (Hz). The Gaunt factor is Draine's fit for
 * the radio to sub-millimetre range, nu_p << nu <~ k_B T / h: it is the
 * classical logarithm at low frequency and tends to 1 at high frequency.
 * Nothing is done about the plasma frequency nu_p = 8.98 kHz sqrt(n_e /
 * cm^-3), below which there is no propagation; at optical frequencies the
 * continuum of an H II region is bound-free and two-photon emission, which
 * this is not.
 *
 * Output: specific intensity, W m^-2 Hz^-1 sr^-1, out[f * npixel + ix * ny +
 * iy] or out[f * nrays + r]. No atomics: the same call on the same state
 * gives the same bits, and a channel's bits do not depend on how many other
 * channels the call has or where in the list it is.
 *
 * Errors, each with a message for cmi_gpu_last_error, before any march and
 * with `out` untouched: CMI_GPU_EINVAL for nf < 1 or nf * npixel (nf * nrays)
 * > 2^28, the cube calls' limit; for a frequency that is not finite and
 * positive; for a kappa that is negative or not finite, an S or a background
 * that is not finite (the fields are counted on the device once uploaded);
 * and everything cmi_gpu_render_field_images or cmi_gpu_render_field_sky
 * refuses for its view or rays. CMI_GPU_ESTATE for the free-free calls
 * without cell data. All calls are synchronous; a call that fails leaves the
 * engine usable.
 *
 * Tuning (cmi_gpu_set_tuning): continuum_channel_block = 4, 8 or 16 channels
 * per march launch; continuum_launch_rays = sample rays or rays per march
 * launch (0: the images' and the sky maps' own bounds). Neither changes a
 * bit of the result. */

/* The free-free {kappa, S} of the cells at freq[nf]: host arrays [nf][ncell]
 * in the engine's cell order - what the free-free calls below march. */
int cmi_gpu_free_free_coefficients(cmi_gpu_engine *engine, int32_t nf,
                                   const double *freq, double *kappa_out,
                                   double *source_out);

/* Free-free images of the parallel camera; view arguments as in
 * cmi_gpu_render_field_images. */
int cmi_gpu_render_continuum_images(cmi_gpu_engine *engine, int32_t nf,
                                    const double *freq,
                                    const double *background /* [nf] or NULL */,
                                    double theta, double phi, int32_t nx,
                                    int32_t ny, const double anchor[2],
                                    const double sides[2], int32_t supersample,
                                    double *out /* [nf][nx][ny] */);

/* The general solver: kappa[nf][ncell], source[nf][ncell] (host) in the
 * engine's cell order. Frequencies are the caller's concern. Needs only
 * cmi_gpu_create. */
int cmi_gpu_render_field_continuum_images(
    cmi_gpu_engine *engine, int32_t nf, const double *kappa,
    const double *source, const double *background /* [nf] or NULL */,
    double theta, double phi, int32_t nx, int32_t ny, const double anchor[2],
    const double sides[2], int32_t supersample,
    double *out /* [nf][nx][ny] */);

/* Free-free along rays from a point; origin and rays as in
 * cmi_gpu_render_field_sky. */
int cmi_gpu_render_continuum_sky(cmi_gpu_engine *engine, int32_t nf,
                                 const double *freq, const double *background,
                                 const double origin[3], int64_t nrays,
                                 const double *directions,
                                 double *out /* [nf][nrays] */);

int cmi_gpu_render_field_continuum_sky(cmi_gpu_engine *engine, int32_t nf,
                                       const double *kappa,
                                       const double *source,
                                       const double *background,
                                       const double origin[3], int64_t nrays,
                                       const double *directions,
                                       double *out /* [nf][nrays] */);

/* The equirectangular map of cmi_gpu_render_line_sky_map in free-free: the
 * same pixel centres and the same 8 x 8 tile order of the rays, lon_range =
 * {lon_min, lon_max}, lat_range likewise; out[f * nlon * nlat + i * nlat +
 * j]. Equals cmi_gpu_render_continuum_sky on the map's directions, bit for
 * bit. */
int cmi_gpu_render_continuum_sky_map(cmi_gpu_engine *engine, int32_t nf,
                                     const double *freq,
                                     const double *background,
                                     const double origin[3], int32_t nlon,
                                     int32_t nlat, const double lon_range[2],
                                     const double lat_range[2],
                                     const double frame[9], double *out);

/* Test hook: the march of n <= 2^20 chosen rays through the caller's fields
 * (nf <= 1024), cell by cell. point == 0: the parallel camera, view = {theta,
 * phi} and rays[n][2] image coordinates as in cmi_gpu_line_image_probe;
 * point == 1: view = the origin[3] and rays[n][3] directions as in
 * cmi_gpu_sky_probe. Row k of `out` has 3 + (2 + nf) * max_cells + nf doubles:
 * {t0, t1, steps, cells[max_cells], ds[max_cells], I[nf][max_cells],
 * I_end[nf]}; t0, t1 and the cell list are the geometry probes', I[f][i] is
 * I_f after step i (for point == 1 before the background is added) and
 * I_end[f] what the render call returns. A ray that misses has NaN, NaN, 0
 * and I_end = bg. A tolerance failure can be traced to a cell from this
 * without running a kernel under a tool. */
int cmi_gpu_continuum_probe(cmi_gpu_engine *engine, int32_t nf,
                            const double *kappa, const double *source,
                            const double *background, int32_t point,
                            const double *view, int64_t n, const double *rays,
                            int32_t max_cells, double *out);

/* ----------------------------------------------- absorbing line cubes -- */
/* A spectral line whose opacity has the line profile, with an optional
 * continuum in the same cells, and the 21-cm line of neutral hydrogen as its
 * first client: the position-velocity cube of H I emission, H I
 * self-absorption and H I absorption against the continuum of the H II region
 * itself. The spectral line cubes and sky cubes above resolve emission in
 * velocity but attenuate all channels with one grey exp(-k ds); the continuum
 * images have an opacity per channel but no profile. No counterpart in the
 * reference.
 *
 * Per cell (host arrays [ncell] in the engine's cell order for the general
 * calls):
 *   a         the line opacity integrated over velocity, m^-1 m s^-1; finite,
 *             >= 0, and a / dv finite
 *   sl        the line source function, W m^-2 Hz^-1 sr^-1; finite
 *   b         the Gaussian width sqrt(2) sigma, m s^-1; finite, >= 0
 *   velocity  [3][ncell], finite; NULL: at rest
 *   kc, sc    a continuum absorption coefficient (m^-1, finite, >= 0) and
 *             source function (finite, and sl - sc finite) that are constant
 *             over the cube's band; both NULL: none
 * and background[nchan] (finite; NULL: all zero).
 *
 * Channels: those of the cubes, nchan equal channels over [vmin, vmax), dv =
 * (vmax - vmin) / nchan, e_c = vmin + c * dv, and the fraction of a cell's
 * profile in channel c is f_c = 0.5 * (E((e_{c+1} - u) / b) - E((e_c - u) /
 * b)) with the E of "spectral line cubes", b == 0 included. u is that
 * section's for the parallel camera and (v - v_obs) . d of "sky cubes" for
 * the rays from a point.
 *
 * Per cell with path ds and per channel, every operation one IEEE operation
 * (-ffp-contract=off) in this order:
 *   al = (a / dv) * f_c;  kappa = al + kc
 *   kappa == 0: the channel is left as it is
 *   w = al / kappa;  S = sc + w * (sl - sc);  em = expm1(-(kappa * ds))
 *   parallel camera (far side to near side, I starts at bg_c):
 *     I = I + em * (I - S)
 *   rays from a point (observer outwards, T = 1 and I = 0 at the start):
 *     I = I + T * (S * -em);  T = T + T * em
 *     and I + T * bg_c behind the last cell, or for a ray that misses.
 * The views, the sample grid and its average, the rays and their checks, the
 * start cell and the step are those of "continuum images". Exact
 * consequences: a == 0 gives kappa == kc and S == sc, so that every channel is
 * cmi_gpu_render_field_continuum_images (_sky) of {kc, sc} with nf = 1, bit
 * for bit; sl == sc == I stays I (parallel camera); and a channel's bits
 * depend on (vmin, dv, c) and the cells only - not on nchan, on the block of
 * channels a launch marches or on the chunking of rays. A cell in which every
 * channel of a launch has f_c == 0 exactly (all of its edges at or beyond 6 b
 * on one side of u) is marched with one expm1 for all of them, kappa = kc and
 * S = sc + 0 * (sl - sc), and skipped when kc == 0 as well: those are the
 * bits of the update above, not an approximation of it.
 *
 * The 21-cm line of the cells as they are (constants h, k_B, c, m_u of the
 * engine): nu_10 = 1420405751.768 Hz, A_10 = 2.8843e-15 s^-1,
 *   C_HI = 3 h c^3 A_10 / (32 pi k_B nu_10^2) = 5.516606267115072e-20 K m^3
 *          s^-1 (1 K km s^-1 of thin emission is 1.8127e18 atoms cm^-2),
 *   n_HI = n * x_H0,  a = C_HI * n_HI / T_s,
 *   sl = (2 * h * nu_10^3 / (c * c)) / expm1((h * nu_10) / (k_B * T_s)),
 *   b = sqrt(2 * (k_B * T / (A_H * m_u) + sigma_turb * sigma_turb)), A_H =
 *       1.00794 (cmi_gpu_emission_line_atomic_weight of HAlpha),
 * T the cell's kinetic temperature. The spin temperature T_s is T
 * (spin_mode 0, spin_temperature ignored), the one value spin_temperature[0]
 * > 0 (spin_mode 1) or spin_temperature[ncell] (spin_mode 2, finite). A cell
 * with n_HI == 0, T <= 0 or T_s <= 0 has a = 0 exactly; sl = 0 for T_s <= 0
 * and the thermal part of b is dropped for T <= 0. With free_free != 0 {kc,
 * sc} are the free-free coefficients of "continuum images" at nu_10, from
 * the same device function; otherwise 0. background_temperature >= 0 gives
 * bg_c = B_nu10(T_bg) in every channel (0 for 0 K), formed on the host.
 * Velocities are those of cmi_gpu_set_cell_velocities.
 *
 * Output: specific intensity averaged over the channel, W m^-2 Hz^-1 sr^-1,
 * out[c * npixel + ix * ny + iy] or out[c * nrays + r]; nchan * npixel (nchan
 * * nrays) <= 2^28.
 *
 * Errors, each with a message for cmi_gpu_last_error, before any march and
 * with `out` untouched: CMI_GPU_EINVAL for everything the cube calls
 * (cmi_gpu_render_field_cube, cmi_gpu_render_field_sky_cube) refuse for
 * their view, rays, velocity axis and velocities and everything the continuum
 * calls refuse; for an a, b or kc that is negative or not finite, an sl, sc
 * or background that is not finite (the fields are counted on the device once
 * uploaded); for kc without sc or the reverse; for a spin temperature or a
 * background temperature out of range; for cells whose 21-cm coefficients do
 * not come out finite (a / dv, b, sl, kc, sc or sl - sc: a spin temperature
 * of 1e-322 K overflows a), counted on the device like the caller's fields,
 * so that the H I calls are held to what the general calls are held to.
 * CMI_GPU_ESTATE for the H I calls without cell data, and for every call of
 * this section, cmi_gpu_hi_coefficients and the probe included, on a block
 * of a decomposed grid. All calls are synchronous; a call that fails leaves
 * the engine usable.
 *
 * Tuning (cmi_gpu_set_tuning): absorbing_cube_channel_block = 4 or 8 channels
 * per march launch; absorbing_cube_expm1_call = 1: the march calls expm1 as a
 * function, 0: it is inlined per channel; absorbing_cube_window_skip = 0: no
 * shortcut for dark cells; absorbing_cube_launch_rays = sample rays or rays
 * per march launch (0: the cubes' own bounds). None changes a bit of the
 * result. */

/* The 21-cm {a, sl, b, kc, sc} of the cells: host arrays [ncell] in the
 * engine's cell order - what the H I calls below march. */
int cmi_gpu_hi_coefficients(cmi_gpu_engine *engine, double sigma_turb,
                            int32_t spin_mode, const double *spin_temperature,
                            int32_t free_free, double *a, double *sl,
                            double *b, double *kc, double *sc);

/* The H I cube of the parallel camera; view arguments as in
 * cmi_gpu_render_field_images. */
int cmi_gpu_render_hi_cube(cmi_gpu_engine *engine, double theta, double phi,
                           int32_t nx, int32_t ny, const double anchor[2],
                           const double sides[2], int32_t supersample,
                           int32_t nchan, double vmin, double vmax,
                           double sigma_turb, int32_t spin_mode,
                           const double *spin_temperature, int32_t free_free,
                           double background_temperature,
                           double *cube /* [nchan][nx][ny] */);

/* H I spectra along rays from a point; origin, observer_velocity (NULL: at
 * rest) and rays as in cmi_gpu_render_field_sky_cube. */
int cmi_gpu_render_hi_sky_cube(cmi_gpu_engine *engine, const double origin[3],
                               const double *observer_velocity, int64_t nrays,
                               const double *directions, int32_t nchan,
                               double vmin, double vmax, double sigma_turb,
                               int32_t spin_mode,
                               const double *spin_temperature,
                               int32_t free_free,
                               double background_temperature,
                               double *out /* [nchan][nrays] */);

/* The longitude-latitude-velocity cube of cmi_gpu_render_line_sky_map_cube in
 * H I: cube[c * nlon * nlat + i * nlat + j]. Equals
 * cmi_gpu_render_hi_sky_cube on the map's directions, bit for bit. */
int cmi_gpu_render_hi_sky_map_cube(
    cmi_gpu_engine *engine, const double origin[3], const double frame[9],
    double lon_min, double lon_max, double lat_min, double lat_max,
    int32_t nlon, int32_t nlat, const double *observer_velocity,
    int32_t nchan, double vmin, double vmax, double sigma_turb,
    int32_t spin_mode, const double *spin_temperature, int32_t free_free,
    double background_temperature, double *cube);

/* The general solver for the parallel camera. Needs only cmi_gpu_create. */
int cmi_gpu_render_field_absorbing_cube(
    cmi_gpu_engine *engine, const double *a, const double *sl,
    const double *b, const double *velocity /* or NULL */,
    const double *kc /* or NULL */, const double *sc /* or NULL */,
    const double *background /* [nchan] or NULL */, double theta, double phi,
    int32_t nx, int32_t ny, const double anchor[2], const double sides[2],
    int32_t supersample, int32_t nchan, double vmin, double vmax,
    double *cube /* [nchan][nx][ny] */);

/* The general solver for rays from a point. */
int cmi_gpu_render_field_absorbing_sky_cube(
    cmi_gpu_engine *engine, const double *a, const double *sl,
    const double *b, const double *velocity, const double *kc,
    const double *sc, const double *background, const double origin[3],
    const double *observer_velocity, int64_t nrays, const double *directions,
    int32_t nchan, double vmin, double vmax, double *out /* [nchan][nrays] */);

/* Test hook: the march of n <= 2^20 chosen rays through the caller's fields
 * (nchan <= 1024), cell by cell, in the style of cmi_gpu_continuum_probe:
 * point == 0, view = {theta, phi}, rays[n][2]; point == 1, view = the
 * origin[3], rays[n][3], observer_velocity as above. Row k of `out` has 3 +
 * (2 + nchan) * max_cells + nchan doubles: {t0, t1, steps, cells[max_cells],
 * ds[max_cells], I[nchan][max_cells], I_end[nchan]}; I[c][i] is I_c after
 * step i (for point == 1 before the background is added) and I_end[c] what
 * the render call returns. The probe runs the update above in every cell,
 * without the shortcut for dark cells. */
int cmi_gpu_absorbing_cube_probe(
    cmi_gpu_engine *engine, const double *a, const double *sl,
    const double *b, const double *velocity, const double *kc,
    const double *sc, const double *background, int32_t nchan, double vmin,
    double vmax, int32_t point, const double *view,
    const double *observer_velocity, int64_t n, const double *rays,
    int32_t max_cells, double *out);

/* ---- absorption spectra ----
 *
 * The optical depth of K resonance lines (1 <= K <= 16) with Voigt profiles
 * along sightlines of finite length, and the column density of each absorber:
 * what UV and optical absorption against a star inside or behind the gas
 * measures. DESIGN.md 4.19 has the reasoning and the figures.
 *
 * Sightlines: ray r is o_r + t d_r, 0 <= t <= L_r. origins[nrays][3] in m,
 * every ray its own; directions[nrays][3] unit vectors, checked as the point
 * camera's are (| |d|^2 - 1 | <= 1e-9, finite); lengths[nrays] in m, L_r > 0,
 * +inf for "to the edge of the box". A ray is clipped to the box and walked
 * as the rays of "sky maps" are (t_start, t_out and the cell-by-cell step of
 * cmi_gpu_sky_probe). t is the running sum of the path lengths ds of the
 * crossings, from t_start. With L_r >= t_out nothing is cut and the (cell,
 * ds) list is cmi_gpu_sky_probe's, exactly; otherwise the crossing with t +
 * ds >= L_r has ds = L_r - t and is the last one. With L_r <= t_start, or
 * when the ray misses the box, the ray contributes nothing: tau = 0, N = 0.
 *
 * Lines: line l has an absorber density n_l[cell] (m^-3), a Doppler width
 * b_l[cell] = sqrt(2) sigma (m s^-1), an integrated cross section in velocity
 * S_l = e^2 f lambda0 / (4 eps0 m_e c) (m^2 m s^-1) and a damping width g_l =
 * Gamma lambda0 / (4 pi) (m s^-1); a = g_l / b_l is the Voigt parameter of a
 * cell. The velocity axis (nchan, vmin, vmax) is the cubes': e_c = vmin + c *
 * dv, centre_c = 0.5 * (e_c + e_{c+1}); velocities are relative to each
 * line's own rest wavelength, lines do not blend.
 *
 * Per crossing of length ds of a cell with n_l != 0 (a cell with n_l == 0
 * contributes nothing, whatever its b), u = (w_x d_x + w_y d_y) + w_z d_z
 * with w = v - v_obs, in this order and without contraction:
 *   nds = n_l * ds;  N = N + nds;  A = nds * S_l
 *   f_c = 0.5 * (E((e_{c+1} - u) / b) - E((e_c - u) / b)),  E of "spectral
 *         line cubes", so that b == 0 is the inclusive step function
 *   g_l == 0:  tau_c = tau_c + A * (f_c / dv)
 *   g_l > 0:   x = (centre_c - u) / b;  wing = Q(g_l / b, x * x) / b
 *              tau_c = tau_c + A * (f_c / dv + wing)
 * Q is the wing term of the Voigt function of "Lyman alpha" (Tasitsiomi
 * 2006: H(a, x) = sqrt(pi) Q + exp(-x^2)), at the channel centre; the
 * Gaussian core is integrated over the channel, so that with g == 0 and an
 * axis that covers the line sum_c tau_c dv = S N. A cell with n_l > 0, g_l >
 * 0 and b_l == 0 has no a: such cells are counted on the device and the call
 * fails with CMI_GPU_EINVAL.
 *
 * Output: tau[(r * K + l) * nchan + c] and N[r * K + l] (m^-2); K * nchan *
 * nrays <= 2^28, nrays <= 2^24. The same call gives the same bits, and a
 * channel's bits depend on (vmin, dv, c), the ray and the cells only: not on
 * nchan, the ray's place in the list or the tuning below.
 *
 * Errors, each before any march and with the outputs untouched:
 * CMI_GPU_EINVAL for K outside 1..16, nchan < 1, vmax <= vmin, directions
 * that are not finite unit vectors, origins that are not finite, L_r <= 0 or
 * NaN, an n, b, S or g that is negative or not finite (n and b are counted on
 * the device), an ion outside 0..13, an atomic weight that is not positive,
 * a null pointer, a periodic box; CMI_GPU_ESTATE on a block of a decomposed
 * grid and for cmi_gpu_render_absorption_spectra without cell data. nrays ==
 * 0 is an empty result (the other arguments are still checked), not an
 * error.
 *
 * Tuning (cmi_gpu_set_tuning): absorption_slab_rows = 1, 2 or 4: a wave
 * takes 64 times as many channels of one ray and line (0, the default: 4, and
 * 1 or 2 for an axis of at most 64 or 128 channels); absorption_edge_sharing
 * = 0: a lane evaluates E at both edges of its channels instead of taking the
 * upper one from its neighbour; absorption_skips = 0: cells whose +-6 b
 * window misses a wave's channels are not skipped. None changes a bit of the
 * result. */

/* The lines are the caller's: n[K][ncell], b[K][ncell], S[K], g[K] and
 * velocity[3][ncell] or NULL (at rest). Needs only cmi_gpu_create. */
int cmi_gpu_render_field_absorption_spectra(
    cmi_gpu_engine *engine, int32_t nlines, const double *n, const double *b,
    const double *S, const double *g, const double *velocity /* or NULL */,
    int64_t nrays, const double *origins, const double *directions,
    const double *lengths, const double *observer_velocity /* or NULL */,
    int32_t nchan, double vmin, double vmax,
    double *tau /* [nrays][K][nchan] */, double *N /* [nrays][K] */);

/* The lines of the engine's own ions: line l absorbs in ion ions[l] (0..13,
 * the order of the ionic fractions) of atomic weight weights[l], with n = n_H
 * * A_element * x_ion (hydrogen's abundance is 1) and b = sqrt(2 * k_B * T /
 * (w * m_u) + 2 * sigma_turb * sigma_turb), the thermal part dropped for T <=
 * 0, built on the device from the cells as they are. Velocities are those of
 * cmi_gpu_set_cell_velocities. */
int cmi_gpu_render_absorption_spectra(
    cmi_gpu_engine *engine, int32_t nlines, const int32_t *ions,
    const double *weights, const double *S, const double *g,
    double sigma_turb, int64_t nrays, const double *origins,
    const double *directions, const double *lengths,
    const double *observer_velocity, int32_t nchan, double vmin, double vmax,
    double *tau, double *N);

/* Test hook: one ray through one line n[ncell], b[ncell], S, g, cell by
 * cell. `out` has 3 + (2 + nprobe) * max_cells + nprobe doubles: {t0, t1,
 * steps, cells[max_cells], ds[max_cells], tau[nprobe][max_cells],
 * tau_end[nprobe]}: t0 = t_start, t1 = t_out (NaN for a ray that misses),
 * the crossings after the cut, tau[k][i] the optical depth of channel
 * channels[k] (nprobe <= 8 of them) after crossing i and tau_end[k] what
 * the render call returns. The probe has no skips. */
int cmi_gpu_absorption_probe(cmi_gpu_engine *engine, const double *n,
                             const double *b, double S, double g,
                             const double *velocity, const double origin[3],
                             const double direction[3], double length,
                             const double *observer_velocity, int32_t nchan,
                             double vmin, double vmax, int32_t nprobe,
                             const int32_t *channels, int32_t max_cells,
                             double *out);

/* ------------------------------------------------------------------------
 * SPH mappings
 *
 * The two linear operators between a cloud of SPH particles and the
 * midpoints of a Cartesian grid that the reference evaluates cell by cell on
 * the host: SPHArrayInterface::operator() / ::write with mapping "centroid"
 * (src/SPHArrayInterface.cpp:931-1075), GadgetSnapshotDensityFunction::
 * operator() (src/GadgetSnapshotDensityFunction.cpp:313-359) and the Phantom
 * / SPHNG density functions without `use new algorithm`
 * (src/PhantomSnapshotDensityFunction.cpp:669-832).
 *
 * Particles: positions p_i [n][3] (m) and smoothing lengths h_i [n] (m,
 * positive). The grid is given in the call - grid_anchor[3], grid_sides[3],
 * ncell[3] - and is NOT the engine's: a decomposed run maps the whole grid
 * on one engine. The midpoint of cell i along an axis is
 * (anchor + side * i) + side / 2 with side = sides / ncell; the cell index is
 * z-fastest as everywhere. Kernel forms W(r, h):
 *   CMI_GPU_SPH_SPLINE_H   the cubic spline of src/CubicSplineKernel.hpp:
 *                          36-59, support h;
 *   CMI_GPU_SPH_SPLINE_2H  the M4 spline of Price 2007
 *                          (PhantomSnapshotDensityFunction::kernel), support
 *                          2 h.
 * The reach of a particle is that support. periodic_box: NULL, or
 * {anchor[3], sides[3]} of a periodic box (m): every separation then takes
 * the minimum image per axis as Box::periodic_distance does, once: if
 * 2 d < -L then d += L; if 2 d >= L then d -= L.
 *
 *   cells <- particles   out[k][c] = sum_i a_k[i] W(|c - p_i|, h_i)
 *       for K <= CMI_GPU_SPH_MAX_AMPLITUDES amplitude arrays
 *       amplitudes[K][n]; out[K][ncells].
 *   particles <- cells   out[i] = sum_c W(|c - p_i|, h_i) g[c]
 *       for one array cell_values g[ncells]; out[n]. With
 *       g_c = (1 - x_c) / cellmass_c this is the reference's inverse
 *       "centroid" mapping: nH_i = 1 - m_i out[i].
 *
 * All pointers are host pointers; the calls are synchronous. Sums are fp64
 * and every output is written by one owner (no floating-point atomics); the
 * order of a cell's terms follows the order the tile lists were filled in,
 * so two calls may differ in the last bits. A pair exactly at the edge of
 * the support has weight 0.
 *
 * A call DECLINES - returns CMI_GPU_EDECLINED, writes nothing, the caller
 * runs its host path - when
 *   CMI_GPU_SPH_DECLINE_NO_PARTICLES  n is 0;
 *   CMI_GPU_SPH_DECLINE_WIDE_KERNEL   a periodic box is given and twice the
 *       largest reach is not below its smallest side (a cell could see two
 *       images of one particle; below that limit the wrapped and the plain
 *       neighbour sets of the host coincide). Without a periodic box the
 *       operator never wraps and never declines for width: a caller whose
 *       host path wraps in a box of its own - the library mode's box of the
 *       particles - applies the rule to that box itself;
 *   CMI_GPU_SPH_DECLINE_LIST_SIZE     the (tile, particle) lists of
 *       cells <- particles would hold more than 2^28 entries (1 GiB).
 *
 * cmi_gpu_get_sph_map_stats, for the last of the two calls on this engine:
 *   [0] tiles of 4 x 8 x 8 cells   [1] (tile, particle) list entries
 *   [2] the longest tile list      [3] records staged through LDS at a time
 *   [4] particles in the wave class [5] in the lane class (particles <- cells:
 *       more than 64 candidate midpoints in the reach box, or up to 64)
 *   [6] 0, or the reason the call declined
 *   [7] device time of the call's kernels in ns, between events: counting,
 *       filling and summing for cells <- particles, the two class kernels
 *       for particles <- cells
 * ([0]-[2] are of cells <- particles, [4]-[5] of particles <- cells.)
 */
enum { CMI_GPU_SPH_SPLINE_H = 0, CMI_GPU_SPH_SPLINE_2H = 1 };
#define CMI_GPU_SPH_MAX_AMPLITUDES 4
enum {
  CMI_GPU_SPH_TAKEN = 0,
  CMI_GPU_SPH_DECLINE_NO_PARTICLES = 1,
  CMI_GPU_SPH_DECLINE_WIDE_KERNEL = 2,
  CMI_GPU_SPH_DECLINE_LIST_SIZE = 3
};
int cmi_gpu_sph_map_to_cells(cmi_gpu_engine *engine, int32_t form, int64_t n,
                             const double *positions, const double *h,
                             int32_t K, const double *amplitudes,
                             const double *periodic_box,
                             const double *grid_anchor,
                             const double *grid_sides, const int32_t *ncell,
                             double *out);
int cmi_gpu_sph_map_to_particles(cmi_gpu_engine *engine, int32_t form,
                                 int64_t n, const double *positions,
                                 const double *h, const double *periodic_box,
                                 const double *grid_anchor,
                                 const double *grid_sides,
                                 const int32_t *ncell,
                                 const double *cell_values, double *out);
int cmi_gpu_get_sph_map_stats(cmi_gpu_engine *engine, int64_t *stats);

#ifdef __cplusplus
}
#endif

#endif /* CMI_GPU_H */
