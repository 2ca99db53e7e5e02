/*
 * engine.hip - host side of the MI355X photoionization engine and its C ABI
 * (include/cmi_gpu.h). Owns the device memory, lowers the plugin descriptors
 * into device tables and launches the kernels of kernels.h on one HIP stream.
 */
#include "../../include/cmi_gpu.h"

#include "atomic_data.h"
#include "linecooling_data.h"
#include "kernels.h"
#include "dust_kernels.h"
#include "line_image_kernels.h"
#include "line_cube_kernels.h"
#include "sky_image_kernels.h"
#include "sky_cube_kernels.h"
#include "dust_cube_kernels.h"
#include "continuum_kernels.h"
#include "absorbing_cube_kernels.h"
#include "lyman_alpha_kernels.h"
#include "sort.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t err__ = (expr);                                                 \
    if (err__ != hipSuccess)                                                   \
      return fail(CMI_GPU_EDEVICE, "%s failed: %s (%s:%d)", #expr,             \
                  hipGetErrorString(err__), __FILE__, __LINE__);               \
  } while (0)
/* ... and for the functions of this file that return a CMI_GPU_* code */
#define CMI_TRY(expr)                                                          \
  do {                                                                         \
    const int rc__ = (expr);                                                   \
    if (rc__)                                                                  \
      return rc__;                                                             \
  } while (0)

struct EventPair {
  hipEvent_t start = nullptr, stop = nullptr;
  uint64_t packets = 0; /* flights started by the launch */
};

} // namespace

struct cmi_gpu_engine {
  cmi_gpu_config config;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int num_cu = 0;

  GridDev grid;
  ModelDev model;
  /* the cells' arrays - through cells_settled() or cells_of_iteration() only:
   * x[2..13] may be pending (metals_pending below) */
  CellsDev cells_unsettled;
  int64_t ncell = 0;

  /* device allocations */
  double *state_block = nullptr;   /* n, T, x[14] : 16 fields */
  double *acc_block = nullptr;     /* J[14], heating[2] : 16 fields */
  bool own_acc = false;
  double2 *opacity = nullptr;
  CountersDev *counters = nullptr;
  TablesDev *tables = nullptr;
  TablesDev *host_tables = nullptr; /* host copy, for host-side tabulation */
  SpectraDev *spectra = nullptr;
  bool spectra_dirty = true; /* cross sections / spectrum changed */
  /* caller-supplied tables (cmi_gpu_set_*_table): [0], [1] the spectra of the
   * discrete / continuous sources, [2] cross sections, [3] recombination
   * rates - device copy {x[n], y[rows][n]} and the host's */
  double *user_table[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<double> user_table_host[4];
  /* counters the host needs between launches: pinned host memory, mapped */
  unsigned int *mailbox = nullptr, *mailbox_dev = nullptr;
  double *source_position = nullptr;
  double *source_cumulative = nullptr;
  std::vector<double> source_position_host;
  double discrete_luminosity = 0., continuous_luminosity = 0.;
  bool have_continuous_spectrum = false;

  bool have_sources = false, have_spectrum = false, have_xsec = false,
       have_recomb = false, have_cells = false;
  bool full_ions = false; /* transport carries all 14 cross sections */
  cmi_gpu_temperature_params tparams;

  /* direction sort of the packet order (keys/ids double buffered) */
  unsigned int *select_count = nullptr; /* block_select_kernel's counter */
  uint32_t *select_ids = nullptr;       /* ... and its list */
  uint64_t select_capacity = 0;
  double *select_rows = nullptr; /* emission rows of a selection, by id */
  uint64_t select_rows_capacity = 0;
  uint32_t *sort_keys[2] = {nullptr, nullptr};
  uint32_t *sort_ids[2] = {nullptr, nullptr};
  void *sort_temp = nullptr;
  size_t sort_temp_bytes = 0;
  uint64_t sort_capacity = 0;
  /* the span cursors of a first-generation launch (ShootArgs::span_cursor) */
  uint32_t *span_cursor = nullptr;
#ifdef CMI_EXPERIMENTS
  /* ShootArgs::phase_clock of the last first-generation launch, and its
   * blocks */
  unsigned long long *phase_clock = nullptr;
  size_t phase_clock_capacity = 0;
  unsigned phase_blocks = 0;
#endif

  /* re-emission queues (ping-pong) */
  double *queue_block = nullptr;
  uint64_t queue_capacity = 0;
  QueueDev ended_queue, ready_queue;
  /* decomposed grids: caller-owned buffer for the flights that leave */
  double *export_rows = nullptr;
  uint64_t export_capacity = 0;
  unsigned int *export_count = nullptr;
  bool own_export_rows = false;
  double *import_rows = nullptr; /* staging for flights given in host memory */
  uint64_t import_capacity = 0;
  unsigned int *queue_counts = nullptr; /* [2]: ended, ready */
  /* tile rounds: two sets of flight rows (in / out of a round), the plan */
  char *tile_block = nullptr;
  uint64_t tile_capacity = 0;
  bool tile_has_weights = false;
  FlightRowsDev tile_rows[2];
  uint32_t *tile_iota = nullptr;
  TileItemDev *tile_items = nullptr;
  uint32_t *tile_begin = nullptr;      /* [ntiles + 2] */
  /* counting sort of the slots by tile (null: too many tiles, radix sort) */
  uint32_t *tile_blockhist = nullptr, *tile_total = nullptr;
  uint32_t *tile_new_slots = nullptr; /* slots filled by a round's re-emissions */
  /* SpectrumTrackers: counted while enabled (the exact marcher then) */
  TrackersDev trackers = {};
  bool trackers_enabled = false;
  /* PAD transport kernels: n x_H inside a layer of ghost cells; whether it
   * holds the records of the cells as they are (whatever writes
   * CellsDev::opacity clears this - pad_records_stale - except the update
   * that writes the padded records itself, hydrogen_update_kernel) */
  double *pad_H = nullptr;
  bool pad_valid = false;
  /* the hydrogen-only update's deferred half: the gates of the last whole-grid
   * update, a bit per cell, and whether x[2..13] have still to be made from
   * them (settle_metal_fractions). Once a pointer to a state field has been
   * handed out (cmi_gpu_field_device_pointer) the engine cannot see every
   * reader and writer any more: no deferral from then on. */
  unsigned long long *metal_gate = nullptr;
  bool metals_pending = false;
  bool state_pointer_escaped = false;
  /* the temperature solve as a pipeline (temperature_pipeline.h) */
  char *temp_pipe_block = nullptr;
  uint32_t temp_pipe_capacity = 0;
  unsigned int *temp_pipe_counts = nullptr;
  uint32_t *tile_ended_slot = nullptr; /* slot of each absorption record */
  uint32_t *tile_ended_pos = nullptr;  /* its position in the next round */
  uint32_t *tile_slot_of[2] = {nullptr, nullptr}; /* position -> slot */
  unsigned int *tile_absorbed_count = nullptr; /* [units of work] */
  unsigned int *tile_absorbed_before = nullptr; /* their running totals */
  unsigned int *tile_counts = nullptr; /* [8]: rows, live, nitems, next item,
                                          absorbed */
  uint64_t tile_rounds_run = 0;
  /* hydrogen-only runs: something other than a transport step may have
   * written one of the accumulator fields such a run never adds to (a field
   * upload, a caller-owned block, a failed clear at a layout switch):
   * cmi_gpu_reset_grid then clears the whole block once */
  bool acc_block_dirty = false;

  struct Tuning {
    bool sort_packets = true;
    int sort_tau_bits = -1;  /* tau classes per direction bin; -1 = auto */
    /* direction bits of the sort key (2 x 11 at most); -1 = auto: one or two
     * fewer than 22 where that saves the radix sort a pass of 8 bits */
    int sort_dir_bits = -1;
    /* the tau classes of every second direction bin the other way round
     * (KeyArgs::class_order); -1 = the default of the run's kind, hydrogen-only
     * or multi-ion (DESIGN_LOG.md 14) */
    int class_order = -1;
    int aggregate = CMI_AGG_BLOCK;      /* first generation (sorted bundles) */
    int aggregate_reemit = CMI_AGG_NONE; /* later generations (random flights) */
    int refill_threshold = CMI_REFILL_THRESHOLD;
    uint32_t chunk = 64;
    int max_blocks_per_cu = 8;
    uint64_t max_packets_per_launch = 1ull << 27;
    int exp_no_atomics = 0;
    bool exact_dda = false;
    bool reemit_passes = true;
    int refill_threshold_reemit = 32;
    /* -1: 4096 on a whole grid; 262144 on a block of a decomposed grid, whose
     * hand-over rounds are many launches of few flights - each costs the
     * latency of its longest flight - (measured on config 5's workload on one
     * GPU, a device per block: 4096 / 32768 / 262144 / 2e6 -> 52 / 47 / 44 /
     * 49 ms per iteration; the blocks' calls in series 360 -> 325 ms) */
    int64_t reemit_inline_below = -1;
    int reemit_max_passes = 12;
    /* later generations in tile rounds (tile_kernels.h) instead of passes of
     * the transport kernel; below tile_min_flights flights the transport
     * kernel finishes them with single atomics */
    bool tile_rounds = true;
    uint64_t tile_min_flights = 100000;
    int tile_min_per_item = -1; /* flights per unit of work; -1 = auto */
    int tile_refill_threshold = 48;
    bool tile_counting_sort = true; /* false: rocPRIM radix sort of the slots */
    /* hydrogen-only cell update: the rows of 64 cells that share one
     * temperature share its temperature-only terms (false: every lane
     * evaluates them for its own cell) */
    bool update_reuse = true;
    /* ... x[2..13] of a whole-grid update made when somebody looks, not in
     * every iteration (hydrogen_update_kernel / metal_fractions_kernel) */
    bool defer_metals = true;
    /* ... and that update writes the padded records of the next transport
     * step itself (false: pad_record_kernel in every cmi_gpu_shoot) */
    bool update_writes_pad = true;
    /* multi-ion runs: the cross sections of re-emitted flights in a kernel of
     * their own (flight_weights_kernel) instead of inside the interaction
     * kernels */
    bool defer_weights = true;
    /* multi-ion runs: the emission physics of the new packets (spectrum,
     * cross sections, optical depth) in the sort-key kernel, read back by the
     * transport kernel (shoot_kernel<..., PRE>) */
    bool pre_emission = true;
    /* hydrogen-only first generation on a whole non-periodic grid: march
     * through the padded records (shoot_kernel<..., PAD>) */
    bool pad_march = true;
    /* sorted first generation: the blocks of an XCD take neighbouring
     * positions of the packet order */
    bool xcd_remap = false;
    /* the temperature solve as a pipeline of kernels (0: one kernel) */
    bool temperature_pipeline = true;
    /* ... whose last slots one launch finishes (temp_finish_kernel: a wave
     * per slot; measured at 256^3, ms per update with 32768 / 8192 / 2048 /
     * 512: 51.2 / 50.7 / 50.7 / 49.8 - the wide steps are the cheaper way
     * while many slots are left) */
    uint32_t temperature_finish_slots = 1024;
    /* the live rows are copied into fresh rows, in tile order, once the
     * flights are spread over this many slots per flight; 0: never; -1: 2 for
     * multi-ion transport (two rows per visit, 25 GB at 1e8 packets: a sparse
     * footprint costs more than the copies), never for hydrogen-only */
    int tile_compact_ratio = -1;
    /* the first generation parks an absorbed packet at the place of its
     * position in the launch's order (no queue counter) */
    bool park_in_place = true;
    /* the kernels with the hydrogen-only block table: how their bundles are
     * scheduled (ShootArgs::span_claim and what follows it; the defaults
     * are what DESIGN_LOG.md 13 measured) */
    bool span_claim = CMI_SPAN_CLAIM_DEFAULT;
    bool emit_before_flush = CMI_EMIT_BEFORE_FLUSH_DEFAULT;
    bool phase_stamps = false; /* experiments build: ShootArgs::phase_clock */
    /* continuum images: channels per march launch (4, 8 or 16) and the rays
     * per launch (0: the images' and the sky maps' own bounds) */
    int continuum_channel_block = CMI_CONTINUUM_FB;
    int64_t continuum_launch_rays = 0;
    int absorbing_cube_channel_block = CMI_ABSORBING_CB;
    int absorbing_cube_expm1_call = CMI_ABSORBING_EXPM1_CALL;
    int absorbing_cube_window_skip = 1;
    int64_t absorbing_cube_launch_rays = 0;
  } tune;

  /* dusty radiative transfer (dust_kernels.h): the kernels' parameters, the
   * image [3][nx][ny], the source's disc CDF, the records {n kappa x_H, 0}
   * and the counters */
  DustDev dust = {};
  double dust_kappa = 0.;
  bool have_dust_scattering = false, have_ccd = false, have_dust_source = false;
  double *dust_image = nullptr;
  double *dust_cdf = nullptr;
  double2 *dust_opacity = nullptr;
  DustCountersDev *dust_counters = nullptr;
  /* dust that follows the gas: records {n sigma, 0}, dust_kappa holds sigma */
  bool dust_per_hydrogen = false;
  /* the cell-luminosity source (DUST_SOURCE_CELLS): its tables, whether they
   * came from the cells (a line source is stale once the cells changed:
   * cells_epoch counts the changes) and the host's copy of the block sums */
  int dust_source = DUST_SOURCE_GALAXY;
  CellSourceDev cell_source = {};
  double *cell_source_cells = nullptr, *cell_source_blocks = nullptr;
  /* cmi_gpu_set_cell_velocities: [3][ncell], m s^-1; null: at rest */
  double *cell_velocities = nullptr;
  std::vector<double> cell_source_blocks_host;
  bool have_cell_source = false, cell_source_from_cells = false;
  uint64_t cells_epoch = 0, cell_source_epoch = 0;
  /* the camera the peel-offs go to (have_ccd: one is set): the parallel
   * camera's parameters are DustDev's, the point camera's these; dust_image
   * is the image of whichever was set last */
  int dust_camera = DUST_CAMERA_PARALLEL;
  SkyCameraDev sky_camera = {};
  /* several views in one run (DUST_CAMERA_PARALLEL_VIEWS, DUST_CAMERA_POINT_
   * VIEWS; dust_nviews is 1 with a single camera): the descriptors on the
   * host and on the device, the per-view counters [nviews][4][slots], the
   * view the camera-dependent probes follow. dust_image is then the stack
   * [nviews][3][pixels]; dust (view 0's fields) and sky_camera (origin and
   * frame of observer 0) carry what the views share. */
  int32_t dust_nviews = 1, dust_probe_view = 0;
  std::vector<DustViewDev> dust_views;
  std::vector<SkyObserverDev> sky_views;
  void *dust_views_dev = nullptr;
  unsigned long long *dust_view_counters = nullptr;
  /* cube mode (cmi_gpu_set_scattered_cube; nchan 0: off): the kernels'
   * argument with the engine's buffers s2 [ncell], obs_velocity [nviews][3]
   * and cube [nviews][3][npixel][nchan], the views the cube was made for, and
   * why it is stale (null: it is not) */
  DustCubeDev dust_cube = {};
  int32_t dust_cube_nviews = 0;
  const char *dust_cube_stale = nullptr;
  /* the line of cmi_gpu_set_cell_source_line */
  int32_t cell_source_line = -1;
  /* Lyman alpha (cmi_gpu_set_lyman_alpha; lya.nchan 0: off): the kernels'
   * argument with the engine's buffers records [ncell], image [nviews]
   * [npixel] and cube [nviews][npixel][nchan], the dust the records were built
   * with, the views, the packet counter of the event loop, and why the mode
   * is stale (null: it is not) */
  LyaDev lya = {};
  DustDev lya_dust = {};
  int32_t lya_nviews = 0;
  unsigned long long *lya_next = nullptr;
  LyaCountersDev *lya_counters = nullptr;
  const char *lya_stale = nullptr;
  /* the radiation field of the mode (cmi_gpu_set_lya_field; null: off): rows
   * [ncell][8], which live and die with the mode */
  double *lya_field = nullptr;

  /* device timing (HIP events around launches) is opt-in: set_tuning
   * ("timing", 1). Events are recycled through a pool; without timing a run
   * of any length creates none. */
  bool timing = false;
  /* with timing: the DDA step counter after every transport launch */
  unsigned long long *launch_steps = nullptr;
  std::vector<EventPair> shoot_events, update_events, kernel_events;
  std::vector<EventPair> event_pool;
};

namespace {

/* The cells' arrays for the iteration's own code - the transport, the
 * hydrogen-only update, the records, the accumulator layout -, which neither
 * reads x[2..13] nor changes what they are made from: nothing is settled. */
inline CellsDev &cells_of_iteration(cmi_gpu_engine *e) {
  return e->cells_unsettled;
}
inline const CellsDev &cells_of_iteration(const cmi_gpu_engine *e) {
  return e->cells_unsettled;
}

int settle_metal_fractions(cmi_gpu_engine *e);

/* A device buffer that only grows: make sure `ptr` holds `want` units, `bytes`
 * in all. The contents are not kept; launches still in flight may read the old
 * buffer, so the stream runs dry before it goes. */
template <class T, class N>
int grow(cmi_gpu_engine *e, T *&ptr, N &capacity, N want, size_t bytes) {
  if (capacity >= want)
    return CMI_GPU_OK;
  HIP_TRY(hipStreamSynchronize(e->stream));
  (void)hipFree(ptr);
  ptr = nullptr;
  capacity = 0;
  HIP_TRY(hipMalloc(&ptr, bytes));
  capacity = want;
  return CMI_GPU_OK;
}

#define CMI_MAX_TIMED_LAUNCHES 65536
/* start / stop of a timed region on the engine's stream; no-ops unless timing
 * is on */
int timer_begin(cmi_gpu_engine *e, EventPair &ev) {
  ev = EventPair();
  if (!e->timing)
    return CMI_GPU_OK;
  if (!e->event_pool.empty()) {
    ev = e->event_pool.back();
    e->event_pool.pop_back();
  } else {
    HIP_TRY(hipEventCreate(&ev.start));
    hipError_t err = hipEventCreate(&ev.stop);
    if (err != hipSuccess) {
      (void)hipEventDestroy(ev.start);
      HIP_TRY(err);
    }
  }
  hipError_t err = hipEventRecord(ev.start, e->stream);
  if (err != hipSuccess) {
    e->event_pool.push_back(ev);
    HIP_TRY(err);
  }
  return CMI_GPU_OK;
}

/* A few counters from device memory into the engine's mailbox - pinned host
 * memory the device writes directly - so that reading them costs a tiny
 * kernel and a stream synchronisation, not a staged copy. */
__global__ void mailbox_kernel(const unsigned int *src, unsigned int *dst,
                               int n) {
  if ((int)threadIdx.x < n)
    dst[threadIdx.x] = src[threadIdx.x];
}
/* the steps counted so far (summed over the shards) */
__global__ void snapshot_steps_kernel(const CountersDev *counters,
                                      unsigned long long *dst) {
  unsigned long long sum = 0;
  for (int k = threadIdx.x; k < CMI_COUNTER_SHARDS; k += 64)
    sum += counters[k].nsteps;
  for (int off = 32; off > 0; off >>= 1)
    sum += __shfl_down(sum, off, 64);
  if (threadIdx.x == 0)
    *dst = sum;
}

/* all shards of the counters, added up (shard k by thread k % 256, then the
 * 256 partial sums in a fixed order: the same result every time) into the
 * engine's mailbox - pinned host memory the device writes directly; a staged
 * copy of the 64 KB of shards into pageable memory cost 0.25 ms */
__global__ void __launch_bounds__(256)
    counters_sum_kernel(const CountersDev *shards, CountersDev *out) {
  __shared__ CountersDev partial[256];
  CountersDev mine = CountersDev();
  for (int k = threadIdx.x; k < CMI_COUNTER_SHARDS; k += 256) {
    const CountersDev c = shards[k];
    mine.totweight += c.totweight;
    for (int i = 0; i < 4; ++i)
      mine.typecount[i] += c.typecount[i];
    mine.nsteps += c.nsteps;
    mine.natomics += c.natomics;
    mine.nwavesteps += c.nwavesteps;
  }
  partial[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    CountersDev sum = CountersDev();
    for (int t = 0; t < 256; ++t) {
      sum.totweight += partial[t].totweight;
      for (int i = 0; i < 4; ++i)
        sum.typecount[i] += partial[t].typecount[i];
      sum.nsteps += partial[t].nsteps;
      sum.natomics += partial[t].natomics;
      sum.nwavesteps += partial[t].nwavesteps;
    }
    *out = sum;
  }
}

static int ensure_mailbox(cmi_gpu_engine *e) {
  if (!e->mailbox) {
    HIP_TRY(hipHostMalloc(&e->mailbox, 16 * sizeof(unsigned int),
                          hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void **)&e->mailbox_dev, e->mailbox, 0));
  }
  return CMI_GPU_OK;
}

static int download_counters(cmi_gpu_engine *e, CountersDev &sum) {
  CMI_TRY(ensure_mailbox(e));
  static_assert(sizeof(CountersDev) <= 16 * sizeof(unsigned int),
                "the counters fit the mailbox");
  counters_sum_kernel<<<1, 256, 0, e->stream>>>(
      e->counters, reinterpret_cast<CountersDev *>(e->mailbox_dev));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  memcpy(&sum, (const void *)e->mailbox, sizeof sum);
  return CMI_GPU_OK;
}

int timer_end(cmi_gpu_engine *e, std::vector<EventPair> &list, EventPair &ev,
              uint64_t packets) {
  if (!ev.start)
    return CMI_GPU_OK;
  ev.packets = packets;
  hipError_t err = hipEventRecord(ev.stop, e->stream);
  if (err != hipSuccess) {
    e->event_pool.push_back(ev);
    HIP_TRY(err);
  }
  /* a caller that never reads its timings does not grow without bound */
  if (list.size() >= CMI_MAX_TIMED_LAUNCHES) {
    e->event_pool.insert(e->event_pool.end(), list.begin(), list.end());
    list.clear();
  }
  if (&list == &e->kernel_events) {
    if (!e->launch_steps)
      HIP_TRY(hipMalloc(&e->launch_steps,
                        sizeof(unsigned long long) * CMI_MAX_TIMED_LAUNCHES));
    snapshot_steps_kernel<<<1, 64, 0, e->stream>>>(
        e->counters, e->launch_steps + list.size());
    HIP_TRY(hipGetLastError());
  }
  list.push_back(ev);
  return CMI_GPU_OK;
}

void release_events(cmi_gpu_engine *e, std::vector<EventPair> &list) {
  e->event_pool.insert(e->event_pool.end(), list.begin(), list.end());
  list.clear();
}

double eV_to_Hz(double eV) {
  /* UnitConverter::to_SI<QUANTITY_FREQUENCY>(eV, "eV"),
   * src/UnitConverter.hpp:156-159,266-300 */
  return eV * CMI_ELECTRONVOLT * (1. / CMI_PLANCK) / 1.;
}

double *field_pointer(cmi_gpu_engine *e, int field) {
  if (field < 0 || field >= CMI_GPU_NFIELD)
    return nullptr;
  if (field < CMI_GPU_FIELD_MEAN_INTENSITY)
    return e->state_block + (int64_t)field * e->ncell;
  const int f = field - CMI_GPU_FIELD_MEAN_INTENSITY;
  if (cells_of_iteration(e).acc_cell_stride != 1) /* [ncell][16], rows in
                                                    * threshold order */
    return e->acc_block + cmi_acc_column(f);
  return e->acc_block + (int64_t)f * cells_of_iteration(e).acc_field_stride;
}

/* element stride of a field: 1 for the state fields, the accumulator layout's
 * cell stride for the accumulator fields */
int64_t field_stride(cmi_gpu_engine *e, int field) {
  return field < CMI_GPU_FIELD_MEAN_INTENSITY
             ? 1
             : cells_of_iteration(e).acc_cell_stride;
}

/* lower the generated raw tables into the device layout, applying the unit
 * conversions of the reference constructors */
void build_tables(TablesDev &t) {
  memset(&t, 0, sizeof t);
  /* src/VernerCrossSections.cpp:36-154 */
  const double eV_to_Hz_fac = CMI_ELECTRONVOLT / CMI_PLANCK;
  static_assert(CMI_VERNER_NTERM == CMI_VERNER_NTERM_DEV, "term count");
  for (int i = 0; i < CMI_VERNER_NTERM; ++i) {
    const cmi_verner_term &raw = cmi_verner_terms[i];
    VernerTermDev &d = t.verner[i];
    d.ion = raw.ion;
    d.shell = raw.shell;
    d.ninn = raw.ninn;
    d.ntot = raw.ntot;
    const double E_th = raw.A[0], E_0 = raw.A[1], sigma_0 = raw.A[2],
                 y_a = raw.A[3], P = raw.A[4], y_w = raw.A[5];
    d.E_th = E_th * eV_to_Hz_fac;
    d.einn = (raw.N < 3) ? 1.e30 : raw.einn_eV * eV_to_Hz_fac;
    d.A_Plconst = 0.5 * P - 5.5 - raw.l;
    d.A_E_0_inv = 1. / (E_0 * eV_to_Hz_fac);
    d.A_sigma_0 = 1.e-22 * sigma_0;
    d.A_y_a_inv = 1. / y_a;
    d.A_P = P;
    d.A_y_w_sq = y_w * y_w;
    d.B_E_0_inv = 1. / (raw.B[2] * eV_to_Hz_fac);
    d.B_sigma_0 = 1.e-22 * raw.B[3];
    d.B_y_a_inv = 1. / raw.B[4];
    d.B_P = raw.B[5];
    d.B_y_w_sq = raw.B[6] * raw.B[6];
    d.B_y_0 = raw.B[7];
    d.B_y_1_sq = raw.B[8] * raw.B[8];
  }
  /* src/VernerRecombinationRates.cpp:38-90 */
  for (int i = 0; i < CMI_VERNER_NREC; ++i) {
    const cmi_verner_rec &raw = cmi_verner_recs[i];
    VernerRecDev &d = t.verner_rec[raw.ion];
    d.kind = raw.kind;
    d.p[0] = raw.p[0];
    d.p[1] = raw.p[1];
    d.p[2] = (raw.kind == 0 && raw.p[2] != 0.) ? 1. / raw.p[2] : raw.p[2];
    d.p[3] = (raw.kind == 0 && raw.p[3] != 0.) ? 1. / raw.p[3] : raw.p[3];
  }
  /* hydrogen and helium: the same fit with their own constants, :165-190 */
  {
    VernerRecDev &h = t.verner_rec[ION_H_n];
    h.kind = 0;
    h.p[0] = 7.982e-11;
    h.p[1] = 0.748;
    h.p[2] = 1. / 3.148;
    h.p[3] = 1. / 7.036e5;
    VernerRecDev &he = t.verner_rec[ION_He_n];
    he.kind = 0;
    he.p[0] = 3.294e-11;
    he.p[1] = 0.691;
    he.p[2] = 1. / 15.54;
    he.p[3] = 1. / 3.676e7;
  }
  /* dielectronic terms: Nussbaumer & Storey (1983) rows {a/t, 1, t, t^2,
   * exponent}, :197-285 */
  auto ns = [&t](int ion, double a, double b, double c, double d, double f) {
    VernerRecDev &r = t.verner_rec[ion];
    r.dkind = 1;
    r.d[0] = a;
    r.d[1] = b;
    r.d[2] = c;
    r.d[3] = d;
    r.d[4] = f;
  };
  ns(ION_C_p1, 1.8267, 4.1012, 4.8443, 0.2261, 0.5960);
  ns(ION_C_p2, 2.3196, 10.7328, 6.8830, -0.1824, 0.4101);
  ns(ION_N_n, 0., 0.6310, 0.1990, -0.0197, 0.4398);
  ns(ION_N_p1, 0.0320, -0.6624, 4.3191, 0.0003, 0.5946);
  ns(ION_N_p2, -0.8806, 11.2406, 30.7066, -1.1721, 0.6127);
  ns(ION_O_n, -0.0001, 0.0001, 0.0956, 0.0193, 0.4106);
  ns(ION_O_p1, -0.0036, 0.7519, 1.5252, -0.0838, 0.2769);
  ns(ION_Ne_p1, 0.0129, -0.1779, 0.9353, -0.0682, 0.4156);
  /* sulphur: sums of exponentials, in eV (:288-303) and in K (:304-312) */
  auto esum = [&t](int ion, double unit, int n, const double *c,
                   const double *E) {
    VernerRecDev &r = t.verner_rec[ion];
    r.dkind = 2;
    r.dunit = unit;
    r.dn = n;
    for (int k = 0; k < n; ++k) {
      r.dc[k] = c[k];
      r.dE[k] = E[k];
    }
  };
  {
    const double c1[] = {1.37e-9}, E1[] = {14.95};
    esum(ION_S_p1, 1. / 1.16045221e4, 1, c1, E1);
    const double c2[] = {8.0729e-9, 1.1012e-10}, E2[] = {17.56, 7.07};
    esum(ION_S_p2, 1. / 1.16045221e4, 2, c2, E2);
    const double c3[] = {5.817e-7, 1.391e-6, 1.123e-5,
                         1.521e-4, 1.875e-3, 2.097e-2};
    const double E3[] = {362.8, 1058., 7160., 3.26e4, 1.235e5, 2.07e5};
    esum(ION_S_p3, 1., 6, c3, E3);
  }
  /* src/ChargeTransferRates.cpp: {kind, a, b, c, d, e, lo, hi};
   * kind 0 zero, 1 constant, 2 a t^b (1 + c e^{d t}), 3 same * e^{e/t},
   * 4 a t^2 */
  auto set = [](CTFitDev &f, int kind, double a, double b, double c, double d,
                double e, double lo, double hi) {
    f.kind = kind;
    f.a = a;
    f.b = b;
    f.c = c;
    f.d = d;
    f.e = e;
    f.lo = lo;
    f.hi = hi;
  };
  /* recombination with H, :44-157 */
  set(t.ct_recomb_H[ION_He_n], 2, 7.47e-21, 2.06, 9.93, -3.89, 0, 0.6, 10.);
  set(t.ct_recomb_H[ION_C_p1], 2, 1.67e-19, 2.79, 304.74, -4.07, 0, 0.5, 5.);
  set(t.ct_recomb_H[ION_C_p2], 2, 3.25e-15, 0.21, 0.19, -3.29, 0, 0.1, 10.);
  set(t.ct_recomb_H[ION_N_n], 2, 1.01e-18, -0.29, -0.92, -8.38, 0, 0.01, 5.);
  set(t.ct_recomb_H[ION_N_p1], 2, 3.05e-16, 0.6, 2.65, -0.93, 0, 0.1, 10.);
  set(t.ct_recomb_H[ION_N_p2], 2, 4.54e-15, 0.57, -0.65, -0.89, 0, 0.001,
      10.);
  set(t.ct_recomb_H[ION_O_n], 2, 1.04e-15, 3.15e-2, -0.61, -9.73, 0, 0.001,
      1.);
  set(t.ct_recomb_H[ION_O_p1], 2, 1.04e-15, 0.27, 2.02, -5.92, 0, 0.01, 10.);
  set(t.ct_recomb_H[ION_Ne_n], 0, 0, 0, 0, 0, 0, 0, 0);
  set(t.ct_recomb_H[ION_Ne_p1], 1, 1.e-20, 0, 0, 0, 0, 0, 0);
  set(t.ct_recomb_H[ION_S_p1], 1, 1.e-20, 0, 0, 0, 0, 0, 0);
  set(t.ct_recomb_H[ION_S_p2], 2, 2.29e-15, 4.02e-2, 1.59, -6.06, 0, 0.1, 3.);
  set(t.ct_recomb_H[ION_S_p3], 2, 6.44e-15, 0.13, 2.69, -5.69, 0, 0.1, 3.);
  /* ionization by H+, :169-250 (all others zero) */
  set(t.ct_ion_H[ION_N_n], 3, 4.55e-18, -0.29, -0.92, -8.38, -1.086, 0.01,
      5.);
  set(t.ct_ion_H[ION_O_n], 3, 7.4e-17, 0.47, 24.37, -0.74, -0.023, 0.001, 1.);
  /* recombination with He, :262-395 */
  set(t.ct_recomb_He[ION_C_p2], 4, 4.6e-17, 0, 0, 0, 0, 0.1, 3.);
  set(t.ct_recomb_He[ION_N_p1], 2, 3.3e-16, 0.29, 1.3, -4.5, 0, 0.1, 3.);
  set(t.ct_recomb_He[ION_N_p2], 1, 1.5e-16, 0, 0, 0, 0, 0, 0);
  set(t.ct_recomb_He[ION_O_p1], 2, 2.e-16, 0.95, 0., 0., 0, 0.5, 5.);
  set(t.ct_recomb_He[ION_Ne_p1], 1, 1.e-20, 0, 0, 0, 0, 0, 0);
  set(t.ct_recomb_He[ION_S_p2], 2, 1.1e-15, 0.56, 0., 0., 0, 0.1, 3.);
  set(t.ct_recomb_He[ION_S_p3], 2, 7.6e-19, 0.32, 3.4, -5.25, 0, 0.1, 3.);

  /* which charge transfer terms the balance of each metal ion contains,
   * src/IonizationStateCalculator.cpp:323-501 */
  {
    const int with_rH[] = {ION_C_p2, ION_N_n,  ION_N_p1, ION_N_p2, ION_O_n,
                           ION_O_p1, ION_Ne_p1, ION_S_p1, ION_S_p2, ION_S_p3};
    for (int ion : with_rH)
      t.metal_ct[ion][0] = t.ct_recomb_H[ion];
    t.metal_ct[ION_N_n][1] = t.ct_ion_H[ION_N_n];
    t.metal_ct[ION_O_n][1] = t.ct_ion_H[ION_O_n];
    const int with_rHe[] = {ION_C_p2,  ION_N_p1, ION_N_p2, ION_O_p1,
                            ION_Ne_p1, ION_S_p2, ION_S_p3};
    for (int ion : with_rHe)
      t.metal_ct[ion][2] = t.ct_recomb_He[ion];
  }

  /* line cooling data, src/LineCoolingData.cpp:42-1399: energy levels to
   * energy differences in K, everything else copied */
  static_assert(CMI_LC_NFIVE == CMI_LC_NFIVE_DEV && CMI_LC_NTWO == CMI_LC_NTWO_DEV,
                "line cooling element counts");
  auto unit_factor = [](int unit) {
    /* :46-61: cm^-1, eV, Ry -> K */
    if (unit == 0)
      return 100. * CMI_PLANCK * CMI_LIGHTSPEED / CMI_BOLTZMANN;
    if (unit == 1)
      return CMI_ELECTRONVOLT / CMI_BOLTZMANN;
    return 2.179872325e-18 / CMI_BOLTZMANN;
  };
  static const int TR[5][5] = {{-1, 0, 1, 2, 3},
                               {-1, -1, 4, 5, 6},
                               {-1, -1, -1, 7, 8},
                               {-1, -1, -1, -1, 9},
                               {-1, -1, -1, -1, -1}};
  LineCoolingDev &lc = t.lc;
  for (int el = 0; el < CMI_LC_NFIVE; ++el) {
    const cmi_lc_five_level &d = cmi_lc_five[el];
    const double f = unit_factor(d.unit);
    for (int j = 1; j < 5; ++j) {
      lc.energy[el][TR[0][j]] = d.levels[j - 1] * f;
      for (int i = 1; i < j; ++i)
        lc.energy[el][TR[i][j]] = (d.levels[j - 1] - d.levels[i - 1]) * f;
    }
    for (int tr = 0; tr < CMI_LC_NTRANS; ++tr) {
      lc.A[el][tr] = d.A[tr];
      for (int k = 0; k < 7; ++k)
        lc.cs[el][tr][k] = d.cs[tr][k];
    }
    for (int k = 0; k < 5; ++k)
      lc.inv_weight[el][k] = d.inv_weight[k];
  }
  for (int el = 0; el < CMI_LC_NTWO; ++el) {
    const cmi_lc_two_level &d = cmi_lc_two[el];
    lc.two_energy[el] = d.energy * unit_factor(d.unit);
    lc.two_A[el] = d.A;
    for (int k = 0; k < 7; ++k)
      lc.two_cs[el][k] = d.cs[k];
    lc.two_inv_weight[el][0] = d.inv_weight[0];
    lc.two_inv_weight[el][1] = d.inv_weight[1];
  }
  /* :1390-1398 */
  lc.prefactor = CMI_PLANCK * CMI_PLANCK /
                 (std::sqrt(CMI_BOLTZMANN) *
                  std::pow(2. * M_PI * CMI_ELECTRON_MASS, 1.5));
}

/* the model as the HOST evaluates it (tabulating spectra, the reference cross
 * section of the sort key): the tables' host copies instead of the device's */
ModelDev host_model_of(const cmi_gpu_engine *e) {
  ModelDev m = e->model;
  m.tables = e->host_tables;
  TableDev *t[4] = {&m.spectrum_table[0], &m.spectrum_table[1], &m.xsec_table,
                    &m.recomb_table};
  for (int k = 0; k < 4; ++k) {
    if (t[k]->n > 0) {
      t[k]->x = e->user_table_host[k].data();
      t[k]->y = e->user_table_host[k].data() + t[k]->n;
    }
  }
  return m;
}

/* store a caller-supplied table: n abscissae and rows x n values */
int store_user_table(cmi_gpu_engine *e, int which, TableDev &t, int32_t n,
                     int rows, const double *x, const double *y,
                     int32_t interpolation) {
  HIP_TRY(hipSetDevice(e->device));
  /* (kernels of an earlier call may still read the old table) */
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<double> &h = e->user_table_host[which];
  h.assign(x, x + n);
  h.insert(h.end(), y, y + (size_t)rows * (size_t)n);
  (void)hipFree(e->user_table[which]);
  e->user_table[which] = nullptr;
  HIP_TRY(hipMalloc(&e->user_table[which], sizeof(double) * h.size()));
  HIP_TRY(hipMemcpy(e->user_table[which], h.data(), sizeof(double) * h.size(),
                    hipMemcpyHostToDevice));
  t.x = e->user_table[which];
  t.y = e->user_table[which] + n;
  t.n = n;
  t.interpolation = interpolation;
  return CMI_GPU_OK;
}

/* n >= 2 abscissae, finite and in strictly ascending order */
bool table_abscissae_ok(int32_t n, const double *x) {
  if (n < 2 || !x)
    return false;
  for (int32_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i]) || (i > 0 && !(x[i] > x[i - 1])))
      return false;
  return true;
}

/* the guide table of a cumulative distribution (SpectraDev) */
void build_guide(const double *cdf, uint16_t *guide) {
  uint32_t last = 0; /* last entry below the current k / G */
  for (uint32_t k = 0; k <= CMI_NGUIDE + 1; ++k) {
    const double edge = (double)k / CMI_NGUIDE;
    while (last + 1 < CMI_NFREQ && cdf[last + 1] < edge)
      ++last;
    guide[k] = (uint16_t)((cdf[last] < edge) ? last : 0u);
  }
}

/* Tabulate the sampled spectra on the host: the constructors of
 * PlanckPhotonSourceSpectrum (src/PlanckPhotonSourceSpectrum.cpp:53-113),
 * Hydrogen/HeliumLymanContinuumSpectrum
 * (src/HydrogenLymanContinuumSpectrum.cpp:40-122,
 * src/HeliumLymanContinuumSpectrum.cpp:45-133) and
 * HeliumTwoPhotonContinuumSpectrum
 * (src/HeliumTwoPhotonContinuumSpectrum.cpp:44-101). */
void build_spectra(const ModelDev &host_model, SpectraDev &s) {
  memset(&s, 0, sizeof s);
  const double h = CMI_PLANCK, k = CMI_BOLTZMANN;
  for (int which_planck = 0; which_planck < 2; ++which_planck) {
    /* 0: the discrete sources' spectrum, 1: the continuous source's */
    const bool wanted =
        which_planck == 0
            ? host_model.spectrum_type == CMI_GPU_SPECTRUM_PLANCK
            : (host_model.continuous_type != 0 &&
               host_model.continuous_spectrum_type == CMI_GPU_SPECTRUM_PLANCK);
    if (!wanted)
      continue;
    const double temperature = which_planck == 0
                                   ? host_model.planck_temperature
                                   : host_model.continuous_planck_temperature;
    double *planck_cdf = which_planck == 0 ? s.planck_cdf : s.planck2_cdf;
    double *planck_logcdf =
        which_planck == 0 ? s.planck_logcdf : s.planck2_logcdf;
    double *planck_logfreq =
        which_planck == 0 ? s.planck_logfreq : s.planck2_logfreq;
    const double max_frequency = 4.;
    const double min_frequency = 3.289e15;
    std::vector<double> frequency(CMI_NFREQ), luminosity(CMI_NFREQ);
    for (int i = 0; i < CMI_NFREQ; ++i) {
      frequency[i] = 1. + i * (max_frequency - 1.) / (CMI_NFREQ - 1.);
      luminosity[i] = frequency[i] * frequency[i] * frequency[i] /
                      (std::exp(h * frequency[i] * min_frequency /
                                (k * temperature)) -
                       1.);
    }
    planck_cdf[0] = 0.;
    for (int i = 1; i < CMI_NFREQ; ++i)
      planck_cdf[i] = planck_cdf[i - 1] +
                        0.5 *
                            (luminosity[i] / frequency[i] +
                             luminosity[i - 1] / frequency[i - 1]) *
                            (frequency[i] - frequency[i - 1]);
    planck_logcdf[0] = -10.;
    planck_logfreq[0] = 0.;
    for (int i = 1; i < CMI_NFREQ; ++i) {
      planck_cdf[i] /= planck_cdf[CMI_NFREQ - 1];
      planck_logcdf[i] = std::log10(planck_cdf[i]);
      planck_logfreq[i] = std::log10(frequency[i]);
    }
  }
  for (int which = 0; which < 2; ++which) {
    const int ion = which == 0 ? ION_H_n : ION_He_n;
    const double min_frequency =
        which == 0 ? 3.289e15 : 1.81 * 3.288465385e15;
    const double max_frequency =
        which == 0 ? 4. * min_frequency : 4. * 3.288465385e15;
    double *nu = s.lyc_freq[which];
    std::vector<double> xsec(CMI_NFREQ);
    for (int i = 0; i < CMI_NFREQ; ++i) {
      nu[i] = min_frequency +
              i * (max_frequency - min_frequency) / (CMI_NFREQ - 1.);
      double sigma[CMI_NION];
      cmi_cross_sections(host_model, nu[i], sigma);
      xsec[i] = sigma[ion];
    }
    for (int iT = 0; iT < CMI_NTEMP; ++iT) {
      double *cdf = s.lyc_cdf[which][iT];
      cdf[0] = 0.;
      s.lyc_T[iT] = 1500. + (iT + 0.5) * 13500. / CMI_NTEMP;
      for (int inu = 1; inu < CMI_NFREQ; ++inu) {
        const double j1 =
            nu[inu - 1] * nu[inu - 1] * nu[inu - 1] * xsec[inu - 1] *
            std::exp(-(h * (nu[inu - 1] - min_frequency)) / (k * s.lyc_T[iT]));
        const double j2 =
            nu[inu] * nu[inu] * nu[inu] * xsec[inu] *
            std::exp(-(h * (nu[inu] - min_frequency)) / (k * s.lyc_T[iT]));
        cdf[inu] =
            0.5 * (j1 / nu[inu] + j2 / nu[inu - 1]) * (nu[inu] - nu[inu - 1]);
      }
      for (int inu = 1; inu < CMI_NFREQ; ++inu)
        cdf[inu] = cdf[inu - 1] + cdf[inu];
      const double total = cdf[CMI_NFREQ - 1];
      for (int inu = 0; inu < CMI_NFREQ; ++inu)
        cdf[inu] /= total; /* NaN rows if the ion's cross section is zero */
    }
  }
  {
    const double min_frequency = 3.288465385e15;
    const double max_frequency = 1.6 * min_frequency;
    const double nu0 = 4.98e15;
    auto A_of = [](double y) {
      if (!(y < 1.))
        return 0.;
      /* Utilities::locate on the 41-point table + linear interpolation */
      uint32_t lo = 0, hi = CMI_HE2Q_N;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (y > cmi_he2q_y[mid])
          lo = mid;
        else
          hi = mid;
      }
      if (lo == CMI_HE2Q_N - 1)
        --lo;
      const double f =
          (y - cmi_he2q_y[lo]) / (cmi_he2q_y[lo + 1] - cmi_he2q_y[lo]);
      return cmi_he2q_A[lo] + f * (cmi_he2q_A[lo + 1] - cmi_he2q_A[lo]);
    };
    for (int i = 0; i < CMI_NFREQ; ++i)
      s.he2pc_freq[i] = min_frequency + i * (max_frequency - min_frequency) /
                                            (CMI_NFREQ - 1.);
    s.he2pc_cdf[0] = 0.;
    for (int i = 1; i < CMI_NFREQ; ++i) {
      const double A1 = A_of(s.he2pc_freq[i - 1] / nu0);
      const double A2 = A_of(s.he2pc_freq[i] / nu0);
      s.he2pc_cdf[i] =
          0.5 * (A1 + A2) * (s.he2pc_freq[i] - s.he2pc_freq[i - 1]);
    }
    for (int i = 1; i < CMI_NFREQ; ++i)
      s.he2pc_cdf[i] = s.he2pc_cdf[i - 1] + s.he2pc_cdf[i];
    const double total = s.he2pc_cdf[CMI_NFREQ - 1];
    for (int i = 0; i < CMI_NFREQ; ++i)
      s.he2pc_cdf[i] /= total;
  }
  build_guide(s.planck_cdf, s.planck_guide);
  build_guide(s.planck2_cdf, s.planck2_guide);
  build_guide(s.he2pc_cdf, s.he2pc_guide);
  for (int which = 0; which < 2; ++which)
    for (int iT = 0; iT < CMI_NTEMP; ++iT)
      build_guide(s.lyc_cdf[which][iT], s.lyc_guide[which][iT]);
}

/* (re)build and upload the spectra tables if a sampled spectrum is in use */
int ensure_spectra(cmi_gpu_engine *e) {
  const bool needed =
      e->model.spectrum_type == CMI_GPU_SPECTRUM_PLANCK ||
      (e->model.continuous_type != 0 &&
       e->model.continuous_spectrum_type == CMI_GPU_SPECTRUM_PLANCK) ||
      e->model.reemit_type == CMI_GPU_REEMIT_PHYSICAL;
  if (!needed || !e->spectra_dirty)
    return CMI_GPU_OK;
  if (!e->spectra)
    HIP_TRY(hipMalloc(&e->spectra, sizeof(SpectraDev)));
  const ModelDev host_model = host_model_of(e);
  SpectraDev *host = new SpectraDev;
  build_spectra(host_model, *host);
  HIP_TRY(hipStreamSynchronize(e->stream));
  hipError_t err =
      hipMemcpy(e->spectra, host, sizeof(SpectraDev), hipMemcpyHostToDevice);
  delete host;
  HIP_TRY(err);
  e->model.spectra = e->spectra;
  e->spectra_dirty = false;
  return CMI_GPU_OK;
}

__global__ void gather_strided_kernel(const double *src, int64_t stride,
                                      double *dst, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += step)
    dst[i] = src[i * stride];
}
__global__ void scatter_strided_kernel(const double *src, double *dst,
                                       int64_t stride, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += step)
    dst[i * stride] = src[i];
}

int grid_blocks(cmi_gpu_engine *e, int64_t work_items, int blocks_per_cu) {
  int64_t want = (work_items + CMI_BLOCK - 1) / CMI_BLOCK;
  int64_t cap = (int64_t)e->num_cu * blocks_per_cu;
  if (want < 1)
    want = 1;
  return (int)(want < cap ? want : cap);
}

int update_full_flag(cmi_gpu_engine *e) {
  /* the light transport kernel is exact iff no ion other than H0 can ever
   * have a non-zero cross section */
  bool full = e->model.xsec_verner != 0;
  if (!full)
    for (int i = 1; i < CMI_NION; ++i)
      if (e->model.xsec_fixed[i] != 0.)
        full = true;
  /* (x[2..13] of a hydrogen-only update are made before the run stops being
   * one) */
  if (full != e->full_ions)
    CMI_TRY(settle_metal_fractions(e));
  /* accumulator layout follows the transport kernel: [16][ncell] when only
   * hydrogen is accumulated (neighbouring cells share 64-B lines), [ncell][16]
   * when every step updates all 16 values of a cell. A switch zeroes the
   * whole block (reset_grid of a hydrogen-only run clears only the fields
   * such a run adds to), so switching between iterations is safe. */
  if (full != e->full_ions && e->acc_block) {
    /* (a clear that could not be enqueued is made up for, with its error
     * reported, by the next cmi_gpu_reset_grid) */
    if (hipSetDevice(e->device) != hipSuccess ||
        hipMemsetAsync(e->acc_block, 0,
                       (size_t)CMI_NACC * e->ncell * sizeof(double),
                       e->stream) != hipSuccess)
      e->acc_block_dirty = true;
  }
  e->full_ions = full;
  CellsDev &cells = cells_of_iteration(e); /* (the layout's strides only) */
  if (full) {
    cells.acc_field_stride = 1;
    cells.acc_cell_stride = CMI_NACC;
  } else {
    cells.acc_field_stride = e->ncell;
    cells.acc_cell_stride = 1;
  }
  return CMI_GPU_OK;
}

/* x[2..13] of the last deferred update, if they are still to be made */
int settle_metal_fractions(cmi_gpu_engine *e) {
  if (!e->metals_pending)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  MetalFractionsArgs a;
  a.model = e->model;
  a.cells = e->cells_unsettled;
  a.count = e->ncell;
  a.gate = e->metal_gate;
  metal_fractions_kernel<<<grid_blocks(e, e->ncell, 8), CMI_BLOCK, 0,
                           e->stream>>>(a, e->tune.update_reuse ? 1 : 0);
  HIP_TRY(hipGetLastError());
  e->metals_pending = false;
  return CMI_GPU_OK;
}

/* The cells' arrays for everybody else - who reads x[2..13], or writes n, T,
 * x[0], x[1] or the model's rates and abundances, which a pending x[2..13] is
 * made from: settled first, which can fail. */
int cells_settled(cmi_gpu_engine *e, CellsDev *&cells) {
  CMI_TRY(settle_metal_fractions(e));
  cells = &e->cells_unsettled;
  return CMI_GPU_OK;
}

/* something other than hydrogen_update_kernel wrote transport records */
inline void pad_records_stale(cmi_gpu_engine *e) { e->pad_valid = false; }

int rebuild_opacity(cmi_gpu_engine *e) {
  pad_records_stale(e);
  opacity_kernel<<<grid_blocks(e, e->ncell, 8), CMI_BLOCK, 0, e->stream>>>(
      cells_of_iteration(e), e->ncell);
  HIP_TRY(hipGetLastError());
  return CMI_GPU_OK;
}

} // namespace

extern "C" {

const char *cmi_gpu_last_error(void) { return g_last_error.c_str(); }

int cmi_gpu_create(const cmi_gpu_config *config, cmi_gpu_engine **out) {
  if (!config || !out)
    return fail(CMI_GPU_EINVAL, "cmi_gpu_create: null argument");
  for (int a = 0; a < 3; ++a) {
    if (config->ncell[a] <= 0)
      return fail(CMI_GPU_EINVAL, "number of cells must be positive");
    if (!(config->sides[a] > 0.))
      return fail(CMI_GPU_EINVAL, "box sides must be positive");
  }
  if (config->sub_ncell[0] > 0 || config->sub_ncell[1] > 0 ||
      config->sub_ncell[2] > 0) {
    for (int a = 0; a < 3; ++a) {
      if (config->sub_ncell[a] < 3 || config->sub_offset[a] < 0 ||
          config->sub_offset[a] + config->sub_ncell[a] > config->ncell[a])
        return fail(CMI_GPU_EINVAL,
                    "a block of a decomposed grid must lie inside the grid "
                    "and be at least 3 cells wide");
    }
  }
  {
    /* the kernels index the cells of an engine with 32 bits (2^31 cells of
     * 272 B would not fit one device anyway); a larger grid has to be
     * decomposed into blocks */
    int64_t local = 1;
    for (int a = 0; a < 3; ++a)
      local *= config->sub_ncell[0] > 0 ? config->sub_ncell[a]
                                        : config->ncell[a];
    if (local >= (1ll << 31))
      return fail(CMI_GPU_EINVAL,
                  "more than 2^31 - 1 cells per engine are not supported");
  }
  int ndev = 0;
  hipError_t err = hipGetDeviceCount(&ndev);
  if (err != hipSuccess || ndev == 0)
    return fail(CMI_GPU_EDEVICE,
                "no HIP device available (%s); this engine has no CPU path",
                err == hipSuccess ? "device count is 0"
                                  : hipGetErrorString(err));
  if (config->device < 0 || config->device >= ndev)
    return fail(CMI_GPU_EINVAL, "device %d out of range [0,%d)",
                config->device, ndev);
  HIP_TRY(hipSetDevice(config->device));

  cmi_gpu_engine *e = new cmi_gpu_engine();
  e->config = *config;
  e->device = config->device;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, e->device));
  e->num_cu = prop.multiProcessorCount;
  if (config->stream) {
    e->stream = (hipStream_t)config->stream;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;
  }

  /* CartesianDensityGrid ctor, src/CartesianDensityGrid.cpp:72-79; a block
   * of a decomposed grid keeps the whole grid's anchor and cell size
   * (DensitySubGridCreator::create_subgrid,
   * src/DensitySubGridCreator.hpp:314-396) */
  GridDev &g = e->grid;
  const bool decomposed = config->sub_ncell[0] > 0 || config->sub_ncell[1] > 0 ||
                          config->sub_ncell[2] > 0;
  for (int a = 0; a < 3; ++a) {
    g.anchor[a] = config->anchor[a];
    g.box_sides[a] = config->sides[a];
    g.global_ncell[a] = config->ncell[a];
    g.ncell[a] = decomposed ? config->sub_ncell[a] : config->ncell[a];
    g.offset[a] = decomposed ? config->sub_offset[a] : 0;
    g.global_periodic[a] = config->periodic[a] ? 1 : 0;
    /* a block of a decomposed grid is not periodic itself: a flight across a
     * periodic face of the whole box is handed over like any other */
    g.periodic[a] = (config->periodic[a] && !decomposed) ? 1 : 0;
    g.cellside[a] = config->sides[a] / config->ncell[a];
    g.inv_cellside[a] = 1. / g.cellside[a];
  }
  g.decomposed = decomposed ? 1 : 0;
  g.copy_rank = 0;
  g.copy_count = 1;
  e->ncell = (int64_t)g.ncell[0] * g.ncell[1] * g.ncell[2];
  g.ncell_total = e->ncell;

  const size_t field_bytes = (size_t)e->ncell * sizeof(double);
  HIP_TRY(hipMalloc(&e->state_block, 16 * field_bytes));
  HIP_TRY(hipMemsetAsync(e->state_block, 0, 16 * field_bytes, e->stream));
  if (config->external_accumulators) {
    e->acc_block = (double *)config->external_accumulators;
  } else {
    HIP_TRY(hipMalloc(&e->acc_block, CMI_NACC * field_bytes));
    e->own_acc = true;
  }
  HIP_TRY(hipMemsetAsync(e->acc_block, 0, CMI_NACC * field_bytes, e->stream));
  HIP_TRY(hipMalloc(&e->opacity, (size_t)e->ncell * sizeof(double2)));
  HIP_TRY(hipMalloc(&e->counters, sizeof(CountersDev) * CMI_COUNTER_SHARDS));
  HIP_TRY(hipMemsetAsync(e->counters, 0,
                         sizeof(CountersDev) * CMI_COUNTER_SHARDS, e->stream));
  HIP_TRY(hipMalloc(&e->tables, sizeof(TablesDev)));
  {
    e->host_tables = new TablesDev;
    build_tables(*e->host_tables);
    HIP_TRY(hipMemcpy(e->tables, e->host_tables, sizeof(TablesDev),
                      hipMemcpyHostToDevice));
  }

  CellsDev &c = cells_of_iteration(e); /* (nothing pending yet) */
  c.number_density = e->state_block;
  c.temperature = e->state_block + e->ncell;
  for (int i = 0; i < CMI_NION; ++i)
    c.x[i] = e->state_block + (int64_t)(2 + i) * e->ncell;
  c.acc_base = e->acc_block;
  c.acc_field_stride = e->ncell; /* SoA until all 16 fields are in use */
  c.acc_cell_stride = 1;
  c.opacity = e->opacity;

  ModelDev &m = e->model;
  memset(&m, 0, sizeof m);
  m.tables = e->tables;
  /* DensityGrid ctor, src/DensityGrid.hpp:219-222 */
  m.nu_H = eV_to_Hz(13.6);
  m.nu_He = eV_to_Hz(24.6);
  m.reemit_type = CMI_GPU_REEMIT_NONE;
  m.photon_weight[0] = 1.;
  m.photon_weight[1] = 1.;

  cmi_gpu_temperature_params &tp = e->tparams;
  tp.do_temperature_calculation = 0;
  tp.minimum_number_of_iterations = 3;
  tp.epsilon_convergence = 1.e-3;
  tp.maximum_number_of_iterations = 100;
  tp.pah_heating_factor = 0.;
  tp.cosmic_ray_heating_factor = 0.;
  tp.cosmic_ray_heating_limit = 0.75;
  tp.cosmic_ray_heating_scale_length = 1.33333 * 3.086e19;
  tp.minimum_ionized_temperature = 4000.;
  m.t_epsilon = tp.epsilon_convergence;
  m.t_max_iterations = tp.maximum_number_of_iterations;
  m.crlim = tp.cosmic_ray_heating_limit;
  m.crscale = tp.cosmic_ray_heating_scale_length;
  m.t_min_ionized = tp.minimum_ionized_temperature;

  HIP_TRY(hipStreamSynchronize(e->stream));
  /* CMI_GPU_TUNING="key=value,key=value": cmi_gpu_set_tuning for hosts that
   * have no way to call it (the cmi-gpu executable, a code that links the
   * library mode): experiments and bisections, not configuration */
  if (const char *env = std::getenv("CMI_GPU_TUNING")) {
    std::string all(env);
    size_t at = 0;
    while (at < all.size()) {
      size_t end = all.find(',', at);
      if (end == std::string::npos)
        end = all.size();
      const std::string item = all.substr(at, end - at);
      const size_t eq = item.find('=');
      if (eq != std::string::npos) {
        const int rc = cmi_gpu_set_tuning(e, item.substr(0, eq).c_str(),
                                          std::atoll(item.c_str() + eq + 1));
        if (rc) {
          cmi_gpu_destroy(e);
          return rc;
        }
      }
      at = end + 1;
    }
  }
  *out = e;
  return CMI_GPU_OK;
}

int cmi_gpu_destroy(cmi_gpu_engine *e) {
  if (!e)
    return CMI_GPU_OK;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  release_events(e, e->shoot_events);
  release_events(e, e->update_events);
  release_events(e, e->kernel_events);
  for (auto &p : e->event_pool) {
    (void)hipEventDestroy(p.start);
    (void)hipEventDestroy(p.stop);
  }
  (void)hipFree(e->state_block);
  if (e->own_acc)
    (void)hipFree(e->acc_block);
  (void)hipFree(e->opacity);
  (void)hipFree(e->counters);
  (void)hipFree(e->trackers.counts);
  (void)hipFree(e->trackers.absorption);
  (void)hipFree(e->trackers.flux);
  (void)hipFree(e->temp_pipe_block);
  (void)hipFree(e->pad_H);
  (void)hipFree(e->metal_gate);
  (void)hipFree(e->temp_pipe_counts);
  (void)hipFree(e->tables);
  (void)hipFree(e->spectra);
  for (int k = 0; k < 4; ++k)
    (void)hipFree(e->user_table[k]);
  delete e->host_tables;
  (void)hipFree(e->source_position);
  (void)hipFree(e->source_cumulative);
  (void)hipFree(e->sort_keys[0]);
  (void)hipFree(e->select_count);
  (void)hipFree(e->span_cursor);
#ifdef CMI_EXPERIMENTS
  (void)hipFree(e->phase_clock);
#endif
  (void)hipFree(e->select_ids);
  (void)hipFree(e->select_rows);
  (void)hipFree(e->sort_temp);
  (void)hipFree(e->queue_block);
  (void)hipFree(e->queue_counts);
  if (e->mailbox)
    (void)hipHostFree(e->mailbox);
  (void)hipFree(e->export_count);
  if (e->own_export_rows)
    (void)hipFree(e->export_rows);
  (void)hipFree(e->import_rows);
  (void)hipFree(e->tile_block);
  (void)hipFree(e->tile_counts);
  (void)hipFree(e->launch_steps);
  (void)hipFree(e->dust_image);
  (void)hipFree(e->dust_views_dev);
  (void)hipFree(e->dust_view_counters);
  (void)hipFree(e->dust_cdf);
  (void)hipFree(e->dust_opacity);
  (void)hipFree(e->dust_counters);
  (void)hipFree(e->cell_source_cells);
  (void)hipFree(e->cell_velocities);
  (void)hipFree(const_cast<double *>(e->dust_cube.s2));
  (void)hipFree(const_cast<double *>(e->dust_cube.obs_velocity));
  (void)hipFree(e->dust_cube.cube);
  (void)hipFree(e->cell_source_blocks);
  (void)hipFree(const_cast<LyaRecord *>(e->lya.records));
  (void)hipFree(e->lya.image);
  (void)hipFree(e->lya.cube);
  (void)hipFree(e->lya_next);
  (void)hipFree(e->lya_counters);
  (void)hipFree(e->lya_field);
  if (e->own_stream)
    (void)hipStreamDestroy(e->stream);
  delete e;
  return CMI_GPU_OK;
}

int cmi_gpu_synchronize(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

int64_t cmi_gpu_number_of_cells(const cmi_gpu_engine *e) {
  return e ? e->ncell : -1;
}

/* PhotonSource ctor, src/PhotonSource.cpp:104-130: how the packets are
 * shared between the discrete sources and the continuous one, and the weight
 * a packet of either kind carries */
static void mix_sources(cmi_gpu_engine *e) {
  ModelDev &m = e->model;
  const double discrete = m.nsource > 0 ? e->discrete_luminosity : 0.;
  const double continuous =
      m.continuous_type != 0 ? e->continuous_luminosity : 0.;
  m.total_luminosity = discrete + continuous;
  m.continuous_probability = 0.;
  m.photon_weight[0] = 1.;
  m.photon_weight[1] = 1.;
  if (m.total_luminosity > 0.) {
    if (discrete > 0.) {
      m.continuous_probability = continuous > 0. ? 0.5 : 0.;
      m.photon_weight[0] = 1.;
      m.photon_weight[1] =
          continuous > 0. ? (1. - m.continuous_probability) * continuous /
                                m.continuous_probability / discrete
                          : 1.;
    } else {
      m.continuous_probability = 1.;
      m.photon_weight[0] = 0.;
      m.photon_weight[1] = 1.;
    }
  }
  e->have_sources = m.total_luminosity > 0.;
}

int cmi_gpu_set_sources(cmi_gpu_engine *e, int32_t n, const double *positions,
                        const double *weights, double total_luminosity) {
  if (!e || n < 0 || (n > 0 && (!positions || !weights)))
    return fail(CMI_GPU_EINVAL, "cmi_gpu_set_sources: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  (void)hipFree(e->source_position);
  (void)hipFree(e->source_cumulative);
  e->source_position = nullptr;
  e->source_cumulative = nullptr;
  e->source_position_host.clear();
  e->model.nsource = 0;
  e->model.source_position = nullptr;
  e->model.source_cumulative = nullptr;
  e->discrete_luminosity = 0.;
  if (n == 0) { /* no discrete sources (a continuous source only) */
    mix_sources(e);
    return CMI_GPU_OK;
  }
  /* PhotonSource ctor, src/PhotonSource.cpp:74-93 */
  std::vector<double> cumulative(n);
  for (int i = 0; i < n; ++i)
    cumulative[i] = (i > 0 ? cumulative[i - 1] : 0.) + weights[i];
  if (std::abs(cumulative.back() - 1.) > 1.e-9) {
    mix_sources(e);
    return fail(CMI_GPU_EINVAL,
                "Discrete source weights do not sum to 1.0 (%g)!",
                cumulative.back());
  }
  cumulative.back() = 1.;
  HIP_TRY(hipMalloc(&e->source_position, sizeof(double) * 3 * n));
  HIP_TRY(hipMalloc(&e->source_cumulative, sizeof(double) * n));
  HIP_TRY(hipMemcpy(e->source_position, positions, sizeof(double) * 3 * n,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->source_cumulative, cumulative.data(),
                    sizeof(double) * n, hipMemcpyHostToDevice));
  e->source_position_host.assign(positions, positions + 3 * (size_t)n);
  e->model.nsource = n;
  e->model.source_position = e->source_position;
  e->model.source_cumulative = e->source_cumulative;
  e->discrete_luminosity = total_luminosity;
  mix_sources(e);
  return CMI_GPU_OK;
}

int cmi_gpu_set_continuous_source(cmi_gpu_engine *e, int32_t type,
                                  double luminosity) {
  if (!e || (type != CMI_GPU_CONTINUOUS_NONE &&
             type != CMI_GPU_CONTINUOUS_ISOTROPIC) ||
      (type != CMI_GPU_CONTINUOUS_NONE && !(luminosity > 0.)))
    return fail(CMI_GPU_EINVAL, "cmi_gpu_set_continuous_source: bad argument");
  e->model.continuous_type = type;
  e->continuous_luminosity = type != CMI_GPU_CONTINUOUS_NONE ? luminosity : 0.;
  e->spectra_dirty = true;
  mix_sources(e);
  return CMI_GPU_OK;
}

int cmi_gpu_set_continuous_source_planar(cmi_gpu_engine *e, int32_t axis,
                                         double intercept,
                                         const double *anchor,
                                         const double *sides,
                                         double luminosity) {
  if (!e || axis < 0 || axis > 2 || !anchor || !sides || !(sides[0] > 0.) ||
      !(sides[1] > 0.) || !(luminosity > 0.))
    return fail(CMI_GPU_EINVAL,
                "cmi_gpu_set_continuous_source_planar: bad argument");
  ModelDev &m = e->model;
  m.continuous_type = CMI_GPU_CONTINUOUS_PLANAR;
  m.continuous_axis = axis;
  m.continuous_intercept = intercept;
  for (int k = 0; k < 2; ++k) {
    m.continuous_anchor[k] = anchor[k];
    m.continuous_side[k] = sides[k];
  }
  e->continuous_luminosity = luminosity;
  e->spectra_dirty = true;
  mix_sources(e);
  return CMI_GPU_OK;
}

int cmi_gpu_set_continuous_spectrum_monochromatic(cmi_gpu_engine *e,
                                                  double frequency) {
  if (!e || !(frequency > 0.))
    return fail(CMI_GPU_EINVAL, "monochromatic spectrum: bad argument");
  e->model.continuous_spectrum_type = CMI_GPU_SPECTRUM_MONOCHROMATIC;
  e->model.continuous_mono_frequency = frequency;
  e->have_continuous_spectrum = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_continuous_spectrum_planck(cmi_gpu_engine *e,
                                           double temperature) {
  if (!e || !(temperature > 0.))
    return fail(CMI_GPU_EINVAL, "Planck spectrum: bad argument");
  e->model.continuous_spectrum_type = CMI_GPU_SPECTRUM_PLANCK;
  e->model.continuous_planck_temperature = temperature;
  e->have_continuous_spectrum = true;
  e->spectra_dirty = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_spectrum_monochromatic(cmi_gpu_engine *e, double frequency) {
  if (!e || !(frequency > 0.))
    return fail(CMI_GPU_EINVAL, "monochromatic spectrum: bad argument");
  e->model.spectrum_type = CMI_GPU_SPECTRUM_MONOCHROMATIC;
  e->model.mono_frequency = frequency;
  e->have_spectrum = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_spectrum_planck(cmi_gpu_engine *e, double temperature) {
  if (!e || !(temperature > 0.))
    return fail(CMI_GPU_EINVAL, "Planck spectrum: bad argument");
  e->model.spectrum_type = CMI_GPU_SPECTRUM_PLANCK;
  e->model.planck_temperature = temperature;
  e->have_spectrum = true;
  e->spectra_dirty = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_spectrum_table(cmi_gpu_engine *e, int32_t role, int32_t n,
                               const double *frequency,
                               const double *cumulative,
                               int32_t interpolation) {
  if (!e || (role != CMI_GPU_ROLE_SOURCE && role != CMI_GPU_ROLE_CONTINUOUS) ||
      !frequency || !table_abscissae_ok(n, cumulative) ||
      (interpolation != CMI_GPU_TABLE_LINEAR &&
       interpolation != CMI_GPU_TABLE_LOGLOG))
    return fail(CMI_GPU_EINVAL,
                "cmi_gpu_set_spectrum_table: needs n >= 2 frequencies and a "
                "strictly ascending cumulative distribution");
  if (cumulative[0] < 0. || cumulative[0] > 1.e-9 ||
      std::abs(cumulative[n - 1] - 1.) > 1.e-9)
    return fail(CMI_GPU_EINVAL,
                "cmi_gpu_set_spectrum_table: the cumulative distribution must "
                "run from 0 to 1 (%g ... %g)",
                cumulative[0], cumulative[n - 1]);
  for (int32_t i = 0; i < n; ++i)
    if (!(frequency[i] > 0.) || !std::isfinite(frequency[i]))
      return fail(CMI_GPU_EINVAL,
                  "cmi_gpu_set_spectrum_table: frequency %d is not positive",
                  i);
  CMI_TRY(store_user_table(e, role, e->model.spectrum_table[role], n, 1,
                           cumulative, frequency, interpolation));
  if (role == CMI_GPU_ROLE_SOURCE) {
    e->model.spectrum_type = CMI_GPU_SPECTRUM_TABLE;
    e->have_spectrum = true;
  } else {
    e->model.continuous_spectrum_type = CMI_GPU_SPECTRUM_TABLE;
    e->have_continuous_spectrum = true;
  }
  return CMI_GPU_OK;
}

int cmi_gpu_set_cross_sections_table(cmi_gpu_engine *e, int32_t n,
                                     const double *frequency,
                                     const double *sigma,
                                     int32_t interpolation) {
  if (!e || !sigma || !table_abscissae_ok(n, frequency) ||
      !(frequency[0] > 0.) ||
      (interpolation != CMI_GPU_TABLE_LINEAR &&
       interpolation != CMI_GPU_TABLE_LOGLOG))
    return fail(CMI_GPU_EINVAL,
                "cmi_gpu_set_cross_sections_table: needs n >= 2 positive, "
                "strictly ascending frequencies and sigma[14][n]");
  for (size_t i = 0; i < (size_t)CMI_NION * (size_t)n; ++i)
    if (!(sigma[i] >= 0.) || !std::isfinite(sigma[i]))
      return fail(CMI_GPU_EINVAL,
                  "cmi_gpu_set_cross_sections_table: cross section %zu of ion "
                  "%zu is negative or not finite",
                  i % (size_t)n, i / (size_t)n);
  CMI_TRY(store_user_table(e, 2, e->model.xsec_table, n, CMI_NION, frequency,
                           sigma, interpolation));
  e->model.xsec_verner = 2;
  e->have_xsec = true;
  e->spectra_dirty = true;
  return update_full_flag(e);
}

int cmi_gpu_set_recombination_rates_table(cmi_gpu_engine *e, int32_t n,
                                          const double *temperature,
                                          const double *alpha,
                                          int32_t interpolation) {
  if (!e || !alpha || !table_abscissae_ok(n, temperature) ||
      !(temperature[0] > 0.) ||
      (interpolation != CMI_GPU_TABLE_LINEAR &&
       interpolation != CMI_GPU_TABLE_LOGLOG))
    return fail(CMI_GPU_EINVAL,
                "cmi_gpu_set_recombination_rates_table: needs n >= 2 positive, "
                "strictly ascending temperatures and alpha[14][n]");
  for (size_t i = 0; i < (size_t)CMI_NION * (size_t)n; ++i)
    if (!(alpha[i] >= 0.) || !std::isfinite(alpha[i]))
      return fail(CMI_GPU_EINVAL,
                  "cmi_gpu_set_recombination_rates_table: rate %zu of ion %zu "
                  "is negative or not finite",
                  i % (size_t)n, i / (size_t)n);
  CMI_TRY(settle_metal_fractions(e)); /* (made from the rates so far) */
  CMI_TRY(store_user_table(e, 3, e->model.recomb_table, n, CMI_NION,
                           temperature, alpha, interpolation));
  e->model.recomb_verner = 2;
  e->have_recomb = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_cross_sections_fixed(cmi_gpu_engine *e, const double *sigma) {
  if (!e || !sigma)
    return fail(CMI_GPU_EINVAL, "fixed cross sections: bad argument");
  e->model.xsec_verner = 0;
  for (int i = 0; i < CMI_NION; ++i)
    e->model.xsec_fixed[i] = sigma[i];
  e->have_xsec = true;
  e->spectra_dirty = true;
  return update_full_flag(e);
}

int cmi_gpu_set_cross_sections_verner(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  e->model.xsec_verner = 1;
  e->have_xsec = true;
  e->spectra_dirty = true;
  return update_full_flag(e);
}

int cmi_gpu_set_recombination_rates_fixed(cmi_gpu_engine *e,
                                          const double *alpha) {
  if (!e || !alpha)
    return fail(CMI_GPU_EINVAL, "fixed recombination rates: bad argument");
  CMI_TRY(settle_metal_fractions(e)); /* (made from the rates so far) */
  e->model.recomb_verner = 0;
  for (int i = 0; i < CMI_NION; ++i)
    e->model.recomb_fixed[i] = alpha[i];
  e->have_recomb = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_recombination_rates_verner(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  CMI_TRY(settle_metal_fractions(e)); /* (made from the rates so far) */
  e->model.recomb_verner = 1;
  e->have_recomb = true;
  return CMI_GPU_OK;
}

int cmi_gpu_set_abundances(cmi_gpu_engine *e, const double *abundances) {
  if (!e || !abundances)
    return fail(CMI_GPU_EINVAL, "abundances: bad argument");
  CMI_TRY(settle_metal_fractions(e)); /* (made with the abundances so far) */
  for (int i = 0; i < 6; ++i)
    e->model.abundance[i] = abundances[i];
  return CMI_GPU_OK;
}

int cmi_gpu_set_reemission(cmi_gpu_engine *e, int32_t type,
                           double fixed_probability, double fixed_frequency) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (type != CMI_GPU_REEMIT_NONE && type != CMI_GPU_REEMIT_PHYSICAL &&
      type != CMI_GPU_REEMIT_FIXED)
    return fail(CMI_GPU_EINVAL,
                "Unknown DiffuseReemissionHandler type: %d", type);
  e->model.reemit_type = type;
  e->spectra_dirty = true;
  e->model.reemit_fixed_probability = fixed_probability;
  e->model.reemit_fixed_frequency = fixed_frequency;
  return CMI_GPU_OK;
}

int cmi_gpu_set_temperature_params(cmi_gpu_engine *e,
                                   const cmi_gpu_temperature_params *params) {
  if (!e || !params)
    return fail(CMI_GPU_EINVAL, "temperature params: bad argument");
  e->tparams = *params;
  ModelDev &m = e->model;
  m.t_epsilon = params->epsilon_convergence;
  m.t_max_iterations = params->maximum_number_of_iterations;
  m.pahfac = params->pah_heating_factor;
  m.crfac = params->cosmic_ray_heating_factor;
  m.crlim = params->cosmic_ray_heating_limit;
  m.crscale = params->cosmic_ray_heating_scale_length;
  m.t_min_ionized = params->minimum_ionized_temperature;
  return CMI_GPU_OK;
}

int cmi_gpu_upload_cells(cmi_gpu_engine *e, const double *number_density,
                         const double *temperature,
                         const double *ionic_fractions) {
  if (!e || !number_density || !temperature)
    return fail(CMI_GPU_EINVAL, "upload_cells: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  ++e->cells_epoch;
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  const size_t bytes = (size_t)e->ncell * sizeof(double);
  HIP_TRY(hipMemcpyAsync(cells->number_density, number_density, bytes,
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(cells->temperature, temperature, bytes,
                         hipMemcpyHostToDevice, e->stream));
  if (ionic_fractions) {
    HIP_TRY(hipMemcpyAsync(cells->x[0], ionic_fractions, CMI_NION * bytes,
                           hipMemcpyHostToDevice, e->stream));
  } else {
    HIP_TRY(hipMemsetAsync(cells->x[0], 0, CMI_NION * bytes, e->stream));
  }
  CMI_TRY(rebuild_opacity(e));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->have_cells = true;
  return CMI_GPU_OK;
}

int cmi_gpu_upload_field(cmi_gpu_engine *e, int32_t field,
                         const double *values) {
  if (!e || !values)
    return fail(CMI_GPU_EINVAL, "upload_field: bad argument");
  double *dst = field_pointer(e, field);
  if (!dst)
    return fail(CMI_GPU_EINVAL, "upload_field: unknown field %d", field);
  HIP_TRY(hipSetDevice(e->device));
  if (field < CMI_GPU_FIELD_MEAN_INTENSITY) {
    ++e->cells_epoch; /* a field of the cells' state */
    /* (pending x[2..13] are those of the state before this upload) */
    CMI_TRY(settle_metal_fractions(e));
  }
  const int64_t stride = field_stride(e, field);
  if (stride == 1) {
    HIP_TRY(hipMemcpyAsync(dst, values, (size_t)e->ncell * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
  } else {
    double *tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (size_t)e->ncell * sizeof(double)));
    hipError_t err = hipMemcpyAsync(tmp, values,
                                    (size_t)e->ncell * sizeof(double),
                                    hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) {
      scatter_strided_kernel<<<grid_blocks(e, e->ncell, 8), CMI_BLOCK, 0,
                               e->stream>>>(tmp, dst, stride, e->ncell);
      err = hipGetLastError();
    }
    if (err == hipSuccess)
      err = hipStreamSynchronize(e->stream);
    (void)hipFree(tmp);
    HIP_TRY(err);
  }
  if (field >= CMI_GPU_FIELD_MEAN_INTENSITY)
    e->acc_block_dirty = true; /* an accumulator field */
  if (field == CMI_GPU_FIELD_NUMBER_DENSITY ||
      field == CMI_GPU_FIELD_IONIC_FRACTION + ION_H_n ||
      field == CMI_GPU_FIELD_IONIC_FRACTION + ION_He_n) {
    CMI_TRY(rebuild_opacity(e));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

int cmi_gpu_download_field(cmi_gpu_engine *e, int32_t field, double *values) {
  if (!e || !values)
    return fail(CMI_GPU_EINVAL, "download_field: bad argument");
  double *src = field_pointer(e, field);
  if (!src)
    return fail(CMI_GPU_EINVAL, "download_field: unknown field %d", field);
  HIP_TRY(hipSetDevice(e->device));
  if (field >= CMI_GPU_FIELD_IONIC_FRACTION + ION_C_p1 &&
      field < CMI_GPU_FIELD_MEAN_INTENSITY)
    CMI_TRY(settle_metal_fractions(e));
  const int64_t stride = field_stride(e, field);
  if (stride == 1) {
    HIP_TRY(hipMemcpyAsync(values, src, (size_t)e->ncell * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  } else {
    double *tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (size_t)e->ncell * sizeof(double)));
    gather_strided_kernel<<<grid_blocks(e, e->ncell, 8), CMI_BLOCK, 0,
                            e->stream>>>(src, stride, tmp, e->ncell);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess)
      err = hipMemcpyAsync(values, tmp, (size_t)e->ncell * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess)
      err = hipStreamSynchronize(e->stream);
    (void)hipFree(tmp);
    HIP_TRY(err);
  }
  return CMI_GPU_OK;
}

int cmi_gpu_accumulator_layout(cmi_gpu_engine *e, int64_t *field_stride_out,
                               int64_t *cell_stride_out) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (field_stride_out)
    *field_stride_out = cells_of_iteration(e).acc_field_stride;
  if (cell_stride_out)
    *cell_stride_out = cells_of_iteration(e).acc_cell_stride;
  return CMI_GPU_OK;
}

void *cmi_gpu_field_device_pointer(cmi_gpu_engine *e, int32_t field) {
  if (!e)
    return nullptr;
  /* a state field in the hands of code the engine cannot see - which may read
   * x[2..13], or write what they are made from, at any time from now on:
   * they are made now and with every update of this engine's from here on */
  if (field >= 0 && field < CMI_GPU_FIELD_MEAN_INTENSITY) {
    if (settle_metal_fractions(e) != CMI_GPU_OK)
      return nullptr;
    e->state_pointer_escaped = true;
  }
  return field_pointer(e, field);
}

int cmi_gpu_get_update_state(cmi_gpu_engine *e, int32_t *metals_pending,
                             int32_t *pad_records_valid,
                             int32_t *deferral_allowed) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (metals_pending)
    *metals_pending = e->metals_pending ? 1 : 0;
  if (pad_records_valid)
    *pad_records_valid = e->pad_valid ? 1 : 0;
  if (deferral_allowed)
    *deferral_allowed =
        (e->tune.defer_metals && !e->state_pointer_escaped) ? 1 : 0;
  return CMI_GPU_OK;
}

int cmi_gpu_reset_grid(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  const size_t field_bytes = (size_t)e->ncell * sizeof(double);
  if (e->full_ions || e->acc_block_dirty) {
    HIP_TRY(hipMemsetAsync(e->acc_block, 0, CMI_NACC * field_bytes,
                           e->stream));
    e->acc_block_dirty = false;
  } else {
    /* hydrogen-only runs add to J_H (and the two heating fields) only - the
     * other thirteen fields of the [16][ncell] block stay as zero as the
     * layout switch left them (update_full_flag); whatever else writes one
     * of them marks the block dirty */
    HIP_TRY(hipMemsetAsync(e->acc_block, 0, field_bytes, e->stream));
    if (e->config.track_heating)
      HIP_TRY(hipMemsetAsync(e->acc_block + (size_t)CMI_NION * e->ncell, 0,
                             2 * field_bytes, e->stream));
  }
  HIP_TRY(hipMemsetAsync(e->counters, 0,
                         sizeof(CountersDev) * CMI_COUNTER_SHARDS, e->stream));
  return CMI_GPU_OK;
}

int cmi_gpu_set_tuning(cmi_gpu_engine *e, const char *key, int64_t value) {
  if (!e || !key)
    return fail(CMI_GPU_EINVAL, "set_tuning: bad argument");
  const std::string k(key);
  if (k == "sort_packets")
    e->tune.sort_packets = value != 0;
  else if (k == "sort_dir_bits")
    e->tune.sort_dir_bits =
        (int)(value < 0 ? -1 : (value < 2 ? 2 : (value > 22 ? 22 : value)));
  else if (k == "sort_tau_bits")
    e->tune.sort_tau_bits = (int)(value < 0 ? -1 : (value > 3 ? 3 : value));
  else if (k == "class_order")
    e->tune.class_order = (int)(value < 0 ? -1 : (value != 0 ? 1 : 0));
  else if (k == "aggregate")
    e->tune.aggregate = (int)(value < 0 ? 0 : (value > 2 ? 2 : value));
  else if (k == "aggregate_reemit")
    e->tune.aggregate_reemit = (int)(value < 0 ? 0 : (value > 2 ? 2 : value));
  else if (k == "refill_threshold")
    e->tune.refill_threshold = (int)(value < 1 ? 1 : (value > 64 ? 64 : value));
  else if (k == "chunk")
    e->tune.chunk = (uint32_t)(value < 64 ? 64 : value);
  else if (k == "max_blocks_per_cu")
    e->tune.max_blocks_per_cu = (int)(value < 1 ? 1 : value);
  else if (k == "max_packets_per_launch")
    e->tune.max_packets_per_launch =
        (uint64_t)(value < 1024 ? 1024 : (value > (1ll << 30) ? (1ll << 30) : value));
  else if (k == "exp_no_atomics")
    e->tune.exp_no_atomics = (int)value;
  else if (k == "exact_dda")
    e->tune.exact_dda = value != 0;
  else if (k == "reemit_passes")
    e->tune.reemit_passes = value != 0;
  else if (k == "refill_threshold_reemit")
    e->tune.refill_threshold_reemit =
        (int)(value < 1 ? 1 : (value > 64 ? 64 : value));
  else if (k == "reemit_inline_below")
    e->tune.reemit_inline_below = value < 0 ? -1 : value;
  else if (k == "reemit_max_passes")
    e->tune.reemit_max_passes = (int)(value < 1 ? 1 : value);
  else if (k == "timing")
    e->timing = value != 0;
  else if (k == "tile_rounds")
    e->tune.tile_rounds = value != 0;
  else if (k == "tile_min_flights")
    e->tune.tile_min_flights = (uint64_t)(value < 0 ? 0 : value);
  else if (k == "tile_min_per_item")
    e->tune.tile_min_per_item = (int)(value < 0 ? -1 : value);
  else if (k == "tile_refill_threshold")
    e->tune.tile_refill_threshold =
        (int)(value < 1 ? 1 : (value > 64 ? 64 : value));
  else if (k == "tile_compact_ratio")
    e->tune.tile_compact_ratio = (int)(value < -1 ? -1 : value);
  else if (k == "park_in_place")
    e->tune.park_in_place = value != 0;
  else if (k == "accumulators_dirty")
    e->acc_block_dirty = e->acc_block_dirty || value != 0;
  else if (k == "temperature_finish_slots")
    e->tune.temperature_finish_slots = (uint32_t)(value < 0 ? 0 : value);
  else if (k == "temperature_pipeline")
    e->tune.temperature_pipeline = value != 0;
  else if (k == "pad_march")
    e->tune.pad_march = value != 0;
  else if (k == "xcd_remap")
    e->tune.xcd_remap = value != 0;
  else if (k == "pre_emission")
    e->tune.pre_emission = value != 0;
  else if (k == "defer_weights")
    e->tune.defer_weights = value != 0;
  else if (k == "tile_counting_sort")
    e->tune.tile_counting_sort = value != 0;
  else if (k == "update_reuse")
    e->tune.update_reuse = value != 0;
  else if (k == "defer_metals")
    e->tune.defer_metals = value != 0;
  else if (k == "update_writes_pad")
    e->tune.update_writes_pad = value != 0;
  else if (k == "span_claim")
    e->tune.span_claim = value != 0;
  else if (k == "emit_before_flush")
    e->tune.emit_before_flush = value != 0;
  else if (k == "phase_stamps")
    e->tune.phase_stamps = value != 0;
  else if (k == "continuum_channel_block") {
    if (value != 4 && value != 8 && value != 16)
      return fail(CMI_GPU_EINVAL, "set_tuning: continuum_channel_block is 4, "
                  "8 or 16 (%lld asked for)", (long long)value);
    e->tune.continuum_channel_block = (int)value;
  } else if (k == "continuum_launch_rays")
    e->tune.continuum_launch_rays = value < 0 ? 0 : value;
  else if (k == "absorbing_cube_channel_block") {
    if (value != 4 && value != 8)
      return fail(CMI_GPU_EINVAL, "set_tuning: absorbing_cube_channel_block "
                  "is 4 or 8 (%lld asked for)", (long long)value);
    e->tune.absorbing_cube_channel_block = (int)value;
  } else if (k == "absorbing_cube_expm1_call")
    e->tune.absorbing_cube_expm1_call = value != 0;
  else if (k == "absorbing_cube_window_skip")
    e->tune.absorbing_cube_window_skip = value != 0;
  else if (k == "absorbing_cube_launch_rays")
    e->tune.absorbing_cube_launch_rays = value < 0 ? 0 : value;
  else
    return fail(CMI_GPU_EINVAL, "set_tuning: unknown key '%s'", key);
  return CMI_GPU_OK;
}

__global__ void iota_kernel(uint32_t *out, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    out[i] = (uint32_t)i;
}

/* n <= 16 counters at `src` (device memory) as they are once the stream has
 * run dry */
static int read_counters(cmi_gpu_engine *e, const unsigned int *src, int n,
                         unsigned int *out) {
  CMI_TRY(ensure_mailbox(e));
  mailbox_kernel<<<1, 16, 0, e->stream>>>(src, e->mailbox_dev, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k)
    out[k] = ((volatile unsigned int *)e->mailbox)[k];
  return CMI_GPU_OK;
}

#include "transport_driver.h"

int cmi_gpu_shoot(cmi_gpu_engine *e, uint32_t seed, uint32_t iteration,
                  uint64_t first_packet, uint64_t n_packets) {
  return shoot_impl(e, seed, iteration, first_packet, n_packets, nullptr);
}

int cmi_gpu_shoot_flights(cmi_gpu_engine *e, uint32_t seed, uint32_t iteration,
                          uint64_t first_packet, const void *flights,
                          uint64_t n_flights) {
  if (!e || (!flights && n_flights))
    return fail(CMI_GPU_EINVAL, "shoot_flights: bad argument");
  if (!e->grid.decomposed)
    return fail(CMI_GPU_ESTATE,
                "shoot_flights: the engine is not a block of a decomposed "
                "grid");
  return shoot_impl(e, seed, iteration, first_packet, n_flights,
                    (const double *)flights);
}

int cmi_gpu_set_export_buffer(cmi_gpu_engine *e, void *rows,
                              uint64_t capacity) {
  if (!e || capacity >= (1ull << 32))
    return fail(CMI_GPU_EINVAL, "set_export_buffer: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (!e->export_count)
    HIP_TRY(hipMalloc(&e->export_count, sizeof(unsigned int)));
  HIP_TRY(hipMemsetAsync(e->export_count, 0, sizeof(unsigned int), e->stream));
  if (e->own_export_rows) {
    (void)hipFree(e->export_rows);
    e->own_export_rows = false;
  }
  e->export_rows = (double *)rows;
  if (!rows && capacity) {
    /* engine-owned buffer, for hosts that exchange through host memory */
    HIP_TRY(hipMalloc(&e->export_rows,
                      sizeof(double) * CMI_FLIGHT_DOUBLES * capacity));
    e->own_export_rows = true;
  }
  e->export_capacity = capacity;
  return CMI_GPU_OK;
}

int cmi_gpu_get_export_count(cmi_gpu_engine *e, uint64_t *count) {
  if (!e || !count)
    return fail(CMI_GPU_EINVAL, "get_export_count: bad argument");
  *count = 0;
  if (!e->export_count)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  unsigned int n = 0;
  HIP_TRY(hipMemcpyAsync(&n, e->export_count, sizeof n, hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (n > e->export_capacity)
    return fail(CMI_GPU_ENOMEM,
                "export buffer overflow: %u flights left the block, room for "
                "%llu - flights were lost, the iteration is invalid",
                n, (unsigned long long)e->export_capacity);
  *count = n;
  return CMI_GPU_OK;
}

int cmi_gpu_download_exports(cmi_gpu_engine *e, double *host_rows,
                             uint64_t capacity, uint64_t *count) {
  if (!e || !count || (!host_rows && capacity))
    return fail(CMI_GPU_EINVAL, "download_exports: bad argument");
  uint64_t n = 0;
  CMI_TRY(cmi_gpu_get_export_count(e, &n));
  *count = n;
  if (n > capacity)
    return fail(CMI_GPU_ENOMEM,
                "download_exports: %llu flights, room for %llu",
                (unsigned long long)n, (unsigned long long)capacity);
  if (n) {
    HIP_TRY(hipMemcpyAsync(host_rows, e->export_rows,
                           sizeof(double) * CMI_FLIGHT_DOUBLES * n,
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return CMI_GPU_OK;
}

int cmi_gpu_shoot_flights_host(cmi_gpu_engine *e, uint32_t seed,
                               uint32_t iteration, uint64_t first_packet,
                               const double *host_rows, uint64_t n_flights) {
  if (!e || (!host_rows && n_flights))
    return fail(CMI_GPU_EINVAL, "shoot_flights_host: bad argument");
  if (n_flights == 0)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  CMI_TRY(grow(e, e->import_rows, e->import_capacity, n_flights,
               sizeof(double) * CMI_FLIGHT_DOUBLES * n_flights));
  /* launches of an earlier call may still read the staging buffer */
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpyAsync(e->import_rows, host_rows,
                         sizeof(double) * CMI_FLIGHT_DOUBLES * n_flights,
                         hipMemcpyHostToDevice, e->stream));
  return cmi_gpu_shoot_flights(e, seed, iteration, first_packet, e->import_rows,
                               n_flights);
}

int cmi_gpu_reset_exports(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (!e->export_count)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemsetAsync(e->export_count, 0, sizeof(unsigned int), e->stream));
  return CMI_GPU_OK;
}

int cmi_gpu_get_counters(cmi_gpu_engine *e, double *totweight,
                         double *typecount, uint64_t *nsteps) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  CountersDev host;
  CMI_TRY(download_counters(e, host));
  if (totweight)
    *totweight = host.totweight;
  if (typecount)
    for (int i = 0; i < 4; ++i)
      typecount[i] = host.typecount[i];
  if (nsteps)
    *nsteps = host.nsteps;
  return CMI_GPU_OK;
}

int cmi_gpu_get_atomic_count(cmi_gpu_engine *e, uint64_t *natomics) {
  if (!e || !natomics)
    return fail(CMI_GPU_EINVAL, "get_atomic_count: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  CountersDev host;
  CMI_TRY(download_counters(e, host));
  *natomics = host.natomics;
  return CMI_GPU_OK;
}

int cmi_gpu_get_phase_clocks(cmi_gpu_engine *e, uint64_t *out,
                             int64_t capacity, int64_t *count) {
  if (!e || !count || capacity < 0 || (!out && capacity))
    return fail(CMI_GPU_EINVAL, "get_phase_clocks: bad argument");
#ifdef CMI_EXPERIMENTS
  if (!e->phase_clock || !e->phase_blocks)
    return fail(CMI_GPU_ESTATE,
                "get_phase_clocks: no launch with phase_stamps yet");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int64_t n = CMI_PHASE_COUNT + 1 + (int64_t)e->phase_blocks;
  *count = n;
  if (capacity)
    HIP_TRY(hipMemcpy(out, e->phase_clock,
                      sizeof(uint64_t) * (size_t)(capacity < n ? capacity : n),
                      hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
#else
  return fail(CMI_GPU_ESTATE,
              "get_phase_clocks: not a build with -DCMI_EXPERIMENTS");
#endif
}

int cmi_gpu_get_wave_steps(cmi_gpu_engine *e, uint64_t *nwavesteps) {
  if (!e || !nwavesteps)
    return fail(CMI_GPU_EINVAL, "get_wave_steps: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  CountersDev host;
  CMI_TRY(download_counters(e, host));
  *nwavesteps = host.nwavesteps;
  return CMI_GPU_OK;
}

/* the temperature solve of the cells [a.first, a.first + a.count) as the
 * pipeline of temperature_pipeline.h, in passes of at most 2^24 cells (the
 * solve state and a step's evaluations of a pass: 10 GB) */
static int temperature_pipeline(cmi_gpu_engine *e, const UpdateArgs &a) {
  const uint32_t want =
      (uint32_t)(a.count < (1ll << 24) ? a.count : (1ll << 24));
  const size_t state_doubles = (size_t)TS_NFIELD;
  const size_t eval_doubles = 3 * (size_t)TE_NFIELD;
  auto bytes_for = [&](uint32_t cap) {
    return sizeof(double) * (state_doubles + eval_doubles) * cap +
           sizeof(uint32_t) * 4 * (size_t)cap;
  };
  CMI_TRY(grow(e, e->temp_pipe_block, e->temp_pipe_capacity, want,
               bytes_for(want)));
  if (!e->temp_pipe_counts)
    HIP_TRY(hipMalloc(&e->temp_pipe_counts, 4 * sizeof(unsigned int)));
  const uint32_t cap = e->temp_pipe_capacity;
  TempPipeArgs p;
  p.u = a;
  p.capacity = cap;
  char *at = e->temp_pipe_block;
  p.state = (double *)at;
  at += sizeof(double) * state_doubles * cap;
  p.eval = (double *)at;
  at += sizeof(double) * eval_doubles * cap;
  p.slot_cell = (uint32_t *)at;
  at += sizeof(uint32_t) * (size_t)cap;
  p.niter = (int32_t *)at;
  at += sizeof(uint32_t) * (size_t)cap;
  p.list[0] = (uint32_t *)at;
  at += sizeof(uint32_t) * (size_t)cap;
  p.list[1] = (uint32_t *)at;
  p.counts = e->temp_pipe_counts;
  for (int64_t done = 0; done < a.count; done += cap) {
    p.chunk_first = a.first + done;
    p.chunk_count = a.count - done < (int64_t)cap ? a.count - done : cap;
    p.current = 0;
    p.nactive = 0;
    HIP_TRY(hipMemsetAsync(p.counts, 0, 4 * sizeof(unsigned int), e->stream));
    temp_begin_kernel<<<grid_blocks(e, p.chunk_count, 8), CMI_BLOCK, 0,
                        e->stream>>>(p);
    HIP_TRY(hipGetLastError());
    unsigned int nactive = 0;
    CMI_TRY(read_counters(e, p.counts, 1, &nactive));
    /* (a solve ends after t_max_iterations steps at the latest) */
    while (nactive != 0) {
      p.nactive = nactive;
      if (nactive <= e->tune.temperature_finish_slots) {
        /* the stragglers: one launch, a wave per slot */
        temp_finish_kernel<<<(unsigned)((64ull * nactive + CMI_BLOCK - 1) /
                                        CMI_BLOCK),
                             CMI_BLOCK, 0, e->stream>>>(p);
        HIP_TRY(hipGetLastError());
        break;
      }
      const int eblocks = grid_blocks(e, 3ll * nactive, 8);
      temp_eval_kernel<<<eblocks, CMI_BLOCK, 0, e->stream>>>(p);
      temp_linecool_kernel<<<eblocks, CMI_BLOCK, 0, e->stream>>>(p);
      unsigned int *next_count = p.counts + 1 + (1 - p.current);
      HIP_TRY(hipMemsetAsync(next_count, 0, sizeof(unsigned int), e->stream));
      temp_secant_kernel<<<grid_blocks(e, (int64_t)nactive, 8), CMI_BLOCK, 0,
                           e->stream>>>(p);
      HIP_TRY(hipGetLastError());
      CMI_TRY(read_counters(e, next_count, 1, &nactive));
      p.current = 1 - p.current;
    }
  }
  return CMI_GPU_OK;
}

int cmi_gpu_update_cells(cmi_gpu_engine *e, uint32_t loop, double totweight) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  return cmi_gpu_update_cells_range(e, loop, totweight, 0, e->ncell);
}

int cmi_gpu_update_cells_range(cmi_gpu_engine *e, uint32_t loop,
                               double totweight, int64_t first_cell,
                               int64_t ncell) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (first_cell < 0 || ncell < 0 || first_cell + ncell > e->ncell)
    return fail(CMI_GPU_EINVAL, "update_cells_range: cells [%lld, %lld) are "
                "not inside the engine's %lld cells", (long long)first_cell,
                (long long)(first_cell + ncell), (long long)e->ncell);
  ++e->cells_epoch;
  if (ncell == 0)
    return CMI_GPU_OK;
  if (!e->have_sources || !e->have_recomb || !e->have_cells)
    return fail(CMI_GPU_ESTATE,
                "cmi_gpu_update_cells: sources, recombination rates and cell "
                "data must be set first");
  if (!(totweight > 0.))
    return fail(CMI_GPU_EINVAL, "update_cells: totweight must be positive");
  HIP_TRY(hipSetDevice(e->device));
  const bool solve_temperature =
      e->tparams.do_temperature_calculation &&
      loop > (uint32_t)e->tparams.minimum_number_of_iterations;
  /* the hydrogen-only update of the whole grid leaves x[2..13] to whoever
   * looks at them first; it replaces whatever an earlier one left pending.
   * Every other update makes the pending ones first: it writes only its own
   * cells, or a temperature they are made from */
  const bool whole = first_cell == 0 && ncell == e->ncell;
  const bool defer = whole && !solve_temperature && !e->full_ions &&
                     e->tune.defer_metals && !e->state_pointer_escaped;
  if (!defer)
    CMI_TRY(settle_metal_fractions(e));
  if (defer && !e->metal_gate)
    HIP_TRY(hipMalloc(&e->metal_gate, sizeof(unsigned long long) *
                                          (size_t)((e->ncell + 63) / 64)));

  UpdateArgs a;
  a.grid = e->grid;
  a.model = e->model;
  a.cells = cells_of_iteration(e);
  /* src/IonizationStateCalculator.cpp:519-522 and :136-137 */
  const double jfac = e->model.total_luminosity / totweight;
  const double hfac = jfac * CMI_PLANCK;
  const double volume =
      e->grid.cellside[0] * e->grid.cellside[1] * e->grid.cellside[2];
  a.jfac = jfac / volume;
  a.hfac = hfac / volume;
  a.first = first_cell;
  a.count = ncell;

  EventPair ev;
  CMI_TRY(timer_begin(e, ev));
  const int blocks = grid_blocks(e, ncell, 8);
  if (defer) {
    HydrogenUpdateArgs h;
    h.u = a;
    h.gate = e->metal_gate;
    /* (the ghost layer is in place from the last pad_records) */
    h.pad_H = (e->pad_valid && e->tune.update_writes_pad) ? e->pad_H : nullptr;
    h.ny = (uint32_t)e->grid.ncell[1];
    h.nz = (uint32_t)e->grid.ncell[2];
    if (!h.pad_H)
      pad_records_stale(e);
    if (e->config.track_heating)
      hydrogen_update_kernel<true><<<blocks, CMI_BLOCK, 0, e->stream>>>(h);
    else
      hydrogen_update_kernel<false><<<blocks, CMI_BLOCK, 0, e->stream>>>(h);
    HIP_TRY(hipGetLastError());
    e->metals_pending = true;
    CMI_TRY(timer_end(e, e->update_events, ev, 0));
    return CMI_GPU_OK;
  }
  pad_records_stale(e); /* (every kernel below writes transport records) */
  if (solve_temperature && e->tune.temperature_pipeline) {
    CMI_TRY(temperature_pipeline(e, a));
  } else if (solve_temperature)
    temperature_kernel<<<blocks, CMI_BLOCK, 0, e->stream>>>(a);
  else if (e->full_ions)
    ionization_kernel<true><<<blocks, CMI_BLOCK, 0, e->stream>>>(a);
  else if (e->config.track_heating)
    ionization_kernel<false, true>
        <<<blocks, CMI_BLOCK, 0, e->stream>>>(a, e->tune.update_reuse ? 1 : 0);
  else
    ionization_kernel<false, false>
        <<<blocks, CMI_BLOCK, 0, e->stream>>>(a, e->tune.update_reuse ? 1 : 0);
  HIP_TRY(hipGetLastError());
  CMI_TRY(timer_end(e, e->update_events, ev, 0));
  return CMI_GPU_OK;
}

int cmi_gpu_compute_emissivities(cmi_gpu_engine *e, int32_t nlines,
                                 const int32_t *lines, int64_t first_cell,
                                 int64_t ncell, double *emissivities) {
  if (!e || !lines || !emissivities)
    return fail(CMI_GPU_EINVAL, "compute_emissivities: null argument");
  if (nlines < 1 || nlines > CMI_NEMISSIONLINE)
    return fail(CMI_GPU_EINVAL, "compute_emissivities: %d lines asked for, "
                "there are %d", (int)nlines, CMI_NEMISSIONLINE);
  if (first_cell < 0 || ncell < 0 || first_cell + ncell > e->ncell)
    return fail(CMI_GPU_EINVAL, "compute_emissivities: cells [%lld, %lld) are "
                "not inside the engine's %lld cells", (long long)first_cell,
                (long long)(first_cell + ncell), (long long)e->ncell);
  if (!e->have_cells)
    return fail(CMI_GPU_ESTATE,
                "compute_emissivities: cell data must be set first");
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  EmissivityArgs a;
  a.model = e->model;
  a.cells = *cells;
  a.first = first_cell;
  a.count = ncell;
  a.nlines = nlines;
  for (int32_t l = 0; l < nlines; ++l) {
    if (lines[l] < 0 || lines[l] >= CMI_NEMISSIONLINE)
      return fail(CMI_GPU_EINVAL, "compute_emissivities: no emission line %d",
                  (int)lines[l]);
    a.lines[l] = lines[l];
  }
  if (ncell == 0)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  double *d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof(double) * (size_t)nlines * (size_t)ncell));
  a.out = d;
  emissivity_kernel<<<grid_blocks(e, ncell, 8), CMI_BLOCK, 0, e->stream>>>(a);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(emissivities, d,
                    sizeof(double) * (size_t)nlines * (size_t)ncell,
                    hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (err != hipSuccess)
    return fail(CMI_GPU_EDEVICE, "compute_emissivities: %s",
                hipGetErrorString(err));
  return CMI_GPU_OK;
}

int cmi_gpu_set_spectrum_trackers(cmi_gpu_engine *e, int32_t n,
                                  const double *positions, int32_t nbins,
                                  const double *opening_angles,
                                  const double *reference_directions) {
  if (n > CMI_MAX_TRACKERS)
    return fail(CMI_GPU_EINVAL, "set_spectrum_trackers: %d trackers, at most "
                "%d", (int)n, CMI_MAX_TRACKERS);
  int32_t bins[CMI_MAX_TRACKERS];
  for (int32_t k = 0; k < n && k < CMI_MAX_TRACKERS; ++k)
    bins[k] = nbins;
  return cmi_gpu_set_trackers(e, n, positions, nullptr, bins, opening_angles,
                              reference_directions);
}

int cmi_gpu_set_trackers(cmi_gpu_engine *e, int32_t n, const double *positions,
                         const int32_t *kinds, const int32_t *nbins,
                         const double *opening_angles,
                         const double *reference_directions) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (n < 0 || n > CMI_MAX_TRACKERS)
    return fail(CMI_GPU_EINVAL, "set_trackers: %d trackers, at most "
                "%d", (int)n, CMI_MAX_TRACKERS);
  if (n > 0 && (!positions || !nbins))
    return fail(CMI_GPU_EINVAL, "set_trackers: bad argument");
  for (int32_t k = 0; k < n; ++k)
    if (nbins[k] < 1)
      return fail(CMI_GPU_EINVAL, "set_trackers: tracker %d with %d bins",
                  (int)k, (int)nbins[k]);
  for (int32_t k = 0; kinds && k < n; ++k)
    if (kinds[k] != CMI_TRACKER_SPECTRUM &&
        kinds[k] != CMI_TRACKER_ABSORPTION && kinds[k] != CMI_TRACKER_WEIGHTED)
      return fail(CMI_GPU_EINVAL, "set_trackers: unknown kind %d of tracker "
                  "%d", (int)kinds[k], (int)k);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  (void)hipFree(e->trackers.counts);
  (void)hipFree(e->trackers.absorption);
  (void)hipFree(e->trackers.flux);
  e->trackers = TrackersDev();
  if (n == 0)
    return CMI_GPU_OK;
  TrackersDev t = TrackersDev();
  t.n = n;
  /* src/SpectrumTracker.hpp:88-90: nbins bins over three Rydberg frequencies */
  t.minimum_frequency = 3.289e15;
  t.first_bin[0] = 0;
  for (int32_t k = 0; k < n; ++k) {
    t.nbins[k] = nbins[k];
    t.first_bin[k + 1] = t.first_bin[k] + nbins[k];
    t.inverse_frequency_width[k] = 1. / (3. * 3.289e15 / nbins[k]);
    if (kinds && kinds[k] == CMI_TRACKER_WEIGHTED) {
      /* LinearFrequencyBins' defaults, src/LinearFrequencyBins.hpp:80-88:
       * from 13.6 eV to 54.4 eV (in Hz: the electronvolt over Planck's
       * constant, src/UnitConverter.hpp:156-159,271 with the values of
       * src/PhysicalConstants.hpp); cmi_gpu_set_tracker_frequency_bins for
       * others */
      const double ev = 1.6021766208e-19 / 6.626070040e-34;
      t.bins_type[k] = CMI_BINS_LINEAR;
      t.bins_min[k] = 13.6 * ev;
      t.bins_max[k] = 54.4 * ev;
      t.inverse_frequency_width[k] = nbins[k] / (t.bins_max[k] - t.bins_min[k]);
    }
  }
  /* LevelFrequencyBins::LevelFrequencyBins, src/LevelFrequencyBins.hpp:52-66:
   * the ionization energies of src/ElementData.hpp:39-105 (Hz) in ascending
   * order, closed by four times hydrogen's */
  {
    const double energies[CMI_NION] = {
        3.28810279e+15, 5.94523574e+15, 5.89588678e+15, 1.15792700e+16,
        3.51435505e+15, 7.15759434e+15, 1.14732262e+16, 3.29284691e+15,
        8.49136314e+15, 5.21432028e+15, 9.90492110e+15, 5.64310422e+15,
        8.41222200e+15, 1.14182796e+16};
    for (int i = 0; i < CMI_NION; ++i)
      t.level_edges[i] = energies[i];
    std::sort(t.level_edges, t.level_edges + CMI_NION);
    t.level_edges[CMI_NION] = 4. * energies[ION_H_n];
  }
  const GridDev &g = e->grid;
  for (int32_t k = 0; k < n; ++k) {
    /* the cell that holds the position (CartesianDensityGrid::get_cell_indices,
     * src/CartesianDensityGrid.cpp:152-161); TrackerManager::add_trackers
     * aborts for a position outside the box (src/TrackerManager.hpp:181-184) */
    int64_t cell = 0;
    bool here = true;
    for (int a = 0; a < 3; ++a) {
      const double x = positions[3 * k + a];
      if (!(x >= g.anchor[a] && x <= g.anchor[a] + g.box_sides[a]))
        return fail(CMI_GPU_EINVAL, "Tracker is not inside grid!");
      int64_t i = (int64_t)((x - g.anchor[a]) * g.inv_cellside[a]);
      if (i >= g.global_ncell[a])
        i = g.global_ncell[a] - 1;
      i -= g.offset[a];
      here = here && i >= 0 && i < g.ncell[a];
      cell = cell * g.ncell[a] + i;
    }
    t.cell[k] = here ? cell : -1;
    t.kind[k] = kinds ? kinds[k] : CMI_TRACKER_SPECTRUM;
    t.cos_opening_angle[k] = opening_angles ? cos(opening_angles[k]) : -1.;
    double norm2 = 0.;
    for (int a = 0; a < 3; ++a) {
      t.direction[k][a] =
          reference_directions ? reference_directions[3 * k + a] : 0.;
      norm2 += t.direction[k][a] * t.direction[k][a];
    }
    if (norm2 > 0.)
      for (int a = 0; a < 3; ++a)
        t.direction[k][a] /= sqrt(norm2);
  }
  const size_t bytes =
      sizeof(unsigned long long) * 3 * (size_t)t.first_bin[n];
  HIP_TRY(hipMalloc(&t.counts, bytes));
  HIP_TRY(hipMemsetAsync(t.counts, 0, bytes, e->stream));
  const size_t abytes = sizeof(double) * 4 * CMI_NION * (size_t)n;
  HIP_TRY(hipMalloc(&t.absorption, abytes));
  HIP_TRY(hipMemsetAsync(t.absorption, 0, abytes, e->stream));
  const size_t fbytes = sizeof(double) * 4 * (size_t)t.first_bin[n];
  HIP_TRY(hipMalloc(&t.flux, fbytes));
  HIP_TRY(hipMemsetAsync(t.flux, 0, fbytes, e->stream));
  e->trackers = t;
  return CMI_GPU_OK;
}

int cmi_gpu_set_tracker_frequency_bins(cmi_gpu_engine *e, int32_t tracker,
                                       int32_t type, double minimum_frequency,
                                       double maximum_frequency) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (tracker < 0 || tracker >= e->trackers.n ||
      e->trackers.kind[tracker] != CMI_TRACKER_WEIGHTED)
    return fail(CMI_GPU_EINVAL, "set_tracker_frequency_bins: tracker %d is "
                "not a weighted spectrum tracker", (int)tracker);
  TrackersDev &t = e->trackers;
  if (type == CMI_BINS_LEVEL) {
    if (t.nbins[tracker] != CMI_NION)
      return fail(CMI_GPU_EINVAL, "set_tracker_frequency_bins: level bins are "
                  "%d bins, tracker %d has %d", CMI_NION, (int)tracker,
                  (int)t.nbins[tracker]);
    t.bins_type[tracker] = CMI_BINS_LEVEL;
    return CMI_GPU_OK;
  }
  if (type != CMI_BINS_LINEAR)
    return fail(CMI_GPU_EINVAL, "Unknown FrequencyBins type: %d", (int)type);
  if (!(maximum_frequency > minimum_frequency))
    return fail(CMI_GPU_EINVAL, "set_tracker_frequency_bins: empty frequency "
                "range");
  t.bins_type[tracker] = CMI_BINS_LINEAR;
  t.bins_min[tracker] = minimum_frequency;
  t.bins_max[tracker] = maximum_frequency;
  t.inverse_frequency_width[tracker] =
      t.nbins[tracker] / (maximum_frequency - minimum_frequency);
  return CMI_GPU_OK;
}

int cmi_gpu_projected_areas(const double *directions, int64_t n,
                            double *areas) {
  if (n < 0 || (n > 0 && (!directions || !areas)))
    return fail(CMI_GPU_EINVAL, "projected_areas: bad argument");
  for (int64_t i = 0; i < n; ++i)
    areas[i] = cmi_projected_area(directions + 3 * i);
  return CMI_GPU_OK;
}

int cmi_gpu_get_tracker_flux(cmi_gpu_engine *e, double *flux) {
  if (!e || !flux)
    return fail(CMI_GPU_EINVAL, "get_tracker_flux: bad argument");
  if (e->trackers.n == 0)
    return fail(CMI_GPU_ESTATE, "get_tracker_flux: no trackers set");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(flux, e->trackers.flux,
                    sizeof(double) * 4 *
                        (size_t)e->trackers.first_bin[e->trackers.n],
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

int cmi_gpu_get_tracker_absorption(cmi_gpu_engine *e, double *absorption) {
  if (!e || !absorption)
    return fail(CMI_GPU_EINVAL, "get_tracker_absorption: bad argument");
  if (e->trackers.n == 0)
    return fail(CMI_GPU_ESTATE, "get_tracker_absorption: no trackers set");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(absorption, e->trackers.absorption,
                    sizeof(double) * 4 * CMI_NION * (size_t)e->trackers.n,
                    hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

int cmi_gpu_enable_trackers(cmi_gpu_engine *e, int32_t enable) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  e->trackers_enabled = enable != 0;
  return CMI_GPU_OK;
}

int cmi_gpu_get_tracker_counts(cmi_gpu_engine *e, uint64_t *counts) {
  if (!e || !counts)
    return fail(CMI_GPU_EINVAL, "get_tracker_counts: bad argument");
  if (e->trackers.n == 0)
    return fail(CMI_GPU_ESTATE, "get_tracker_counts: no trackers set");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(counts, e->trackers.counts,
                         sizeof(unsigned long long) * 3 *
                             (size_t)e->trackers.first_bin[e->trackers.n],
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

int cmi_gpu_refresh_transport_records(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  return rebuild_opacity(e);
}

int cmi_gpu_emit_packets(cmi_gpu_engine *e, uint32_t seed, uint32_t iteration,
                         uint64_t first_packet, uint64_t n, double *position,
                         double *direction, double *frequency,
                         double *cross_sections, double *tau) {
  if (!e || !position || !direction || !frequency || !cross_sections || !tau)
    return fail(CMI_GPU_EINVAL, "emit_packets: bad argument");
  if (!e->have_sources || (e->model.nsource > 0 && !e->have_spectrum) ||
      (e->model.continuous_type != 0 && !e->have_continuous_spectrum) ||
      !e->have_xsec)
    return fail(CMI_GPU_ESTATE, "emit_packets: model not complete");
  if (n == 0)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  CMI_TRY(ensure_spectra(e));
  double *d = nullptr;
  const size_t per = 3 + 3 + 1 + CMI_NION + 1;
  HIP_TRY(hipMalloc(&d, sizeof(double) * per * n));
  double *dpos = d, *ddir = d + 3 * n, *dnu = d + 6 * n, *dsig = d + 7 * n,
         *dtau = d + (7 + CMI_NION) * n;
  emit_probe_kernel<<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
      e->grid, e->model, seed, iteration, first_packet, n, dpos, ddir, dnu,
      dsig, dtau);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(position, dpos, sizeof(double) * 3 * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(direction, ddir, sizeof(double) * 3 * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(frequency, dnu, sizeof(double) * n, hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(cross_sections, dsig, sizeof(double) * CMI_NION * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(tau, dtau, sizeof(double) * n, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

int cmi_gpu_trace_packets(cmi_gpu_engine *e, uint64_t n,
                          const double *position, const double *direction,
                          const double *tau, const double *sigma_H,
                          const double *sigma_He_corr, int32_t max_steps,
                          int64_t *out_cell, double *out_ds,
                          int32_t *out_nsteps, int64_t *out_last_cell,
                          double *out_position) {
  if (!e || !position || !direction || !tau || !sigma_H || !sigma_He_corr ||
      !out_cell || !out_ds || !out_nsteps || !out_last_cell || !out_position ||
      max_steps <= 0)
    return fail(CMI_GPU_EINVAL, "trace_packets: bad argument");
  if (!e->have_cells)
    return fail(CMI_GPU_ESTATE, "trace_packets: no cell data");
  if (n == 0)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  char *buf = nullptr;
  const size_t in_bytes = sizeof(double) * (3 + 3 + 1 + 1 + 1) * n;
  const size_t cell_bytes = sizeof(int64_t) * (size_t)max_steps * n;
  const size_t ds_bytes = sizeof(double) * (size_t)max_steps * n;
  const size_t tail = (sizeof(int64_t) + 3 * sizeof(double)) * n +
                      sizeof(int32_t) * n;
  HIP_TRY(hipMalloc(&buf, in_bytes + cell_bytes + ds_bytes + tail));
  double *dpos = (double *)buf, *ddir = dpos + 3 * n, *dtau = ddir + 3 * n,
         *dsh = dtau + n, *dshe = dsh + n;
  int64_t *dcell = (int64_t *)(buf + in_bytes);
  double *dds = (double *)(buf + in_bytes + cell_bytes);
  int64_t *dlast = (int64_t *)(buf + in_bytes + cell_bytes + ds_bytes);
  double *dfinal = (double *)(dlast + n);
  int32_t *dnsteps = (int32_t *)(dfinal + 3 * n);
  hipError_t err = hipMemcpy(dpos, position, sizeof(double) * 3 * n,
                             hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(ddir, direction, sizeof(double) * 3 * n,
                    hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(dtau, tau, sizeof(double) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(dsh, sigma_H, sizeof(double) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(dshe, sigma_He_corr, sizeof(double) * n,
                    hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemsetAsync(dcell, 0xff, cell_bytes, e->stream);
  if (err == hipSuccess)
    err = hipMemsetAsync(dds, 0, ds_bytes, e->stream);
  if (err == hipSuccess) {
    if (e->tune.exact_dda || e->ncell >= CMI_FAST_MARCHER_MAX_CELLS)
      trace_probe_kernel<true><<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
          e->grid, e->opacity, n, dpos, ddir, dtau, dsh, dshe, max_steps,
          dcell, dds, dnsteps, dlast, dfinal);
    else
      trace_probe_kernel<false>
          <<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
              e->grid, e->opacity, n, dpos, ddir, dtau, dsh, dshe, max_steps,
              dcell, dds, dnsteps, dlast, dfinal);
    err = hipGetLastError();
  }
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(out_cell, dcell, cell_bytes, hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(out_ds, dds, ds_bytes, hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(out_nsteps, dnsteps, sizeof(int32_t) * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(out_last_cell, dlast, sizeof(int64_t) * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(out_position, dfinal, sizeof(double) * 3 * n,
                    hipMemcpyDeviceToHost);
  (void)hipFree(buf);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

int cmi_gpu_sample_spectrum(cmi_gpu_engine *e, int32_t kind,
                            double temperature, uint32_t seed, uint64_t n,
                            double *frequencies) {
  if (!e || !frequencies || kind < 0 || kind > 3)
    return fail(CMI_GPU_EINVAL, "sample_spectrum: bad argument");
  if (!e->have_xsec)
    return fail(CMI_GPU_ESTATE, "sample_spectrum: cross sections not set");
  if (n == 0)
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  /* force the tables even if no sampled spectrum is configured */
  const int32_t saved = e->model.reemit_type;
  e->model.reemit_type = CMI_GPU_REEMIT_PHYSICAL;
  int rc = ensure_spectra(e);
  e->model.reemit_type = saved;
  if (rc)
    return rc;
  if (kind == 0 && e->model.spectrum_type != CMI_GPU_SPECTRUM_PLANCK)
    return fail(CMI_GPU_ESTATE, "sample_spectrum: no Planck spectrum set");
  double *d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof(double) * n));
  spectrum_probe_kernel<<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(
      e->model, kind, temperature, seed, n, d);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(frequencies, d, sizeof(double) * n, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

int cmi_gpu_thermal_probe(cmi_gpu_engine *e, int64_t n, int32_t solve,
                          const double *J, const double *heating,
                          const double *temperature,
                          const double *number_density, double *out_fractions,
                          double *out_temperature, double *out_pair) {
  if (!e || n <= 0 || !J || !heating || !temperature || !number_density ||
      !out_fractions || !out_temperature || !out_pair)
    return fail(CMI_GPU_EINVAL, "thermal_probe: bad argument");
  if (!e->have_recomb)
    return fail(CMI_GPU_ESTATE, "thermal_probe: recombination rates not set");
  HIP_TRY(hipSetDevice(e->device));
  double *d = nullptr;
  const size_t in_count = (size_t)n * (CMI_NION + 2 + 1 + 1);
  const size_t out_count = (size_t)n * (CMI_NION + 1 + 2);
  HIP_TRY(hipMalloc(&d, sizeof(double) * (in_count + out_count)));
  double *dJ = d, *dh = dJ + CMI_NION * n, *dT = dh + 2 * n, *dn = dT + n,
         *dx = dn + n, *dTo = dx + CMI_NION * n, *dp = dTo + n;
  hipError_t err =
      hipMemcpy(dJ, J, sizeof(double) * CMI_NION * n, hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(dh, heating, sizeof(double) * 2 * n, hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(dT, temperature, sizeof(double) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(dn, number_density, sizeof(double) * n,
                    hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    thermal_probe_kernel<<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
        e->model, n, solve, dJ, dh, dT, dn, dx, dTo, dp);
    err = hipGetLastError();
  }
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(out_fractions, dx, sizeof(double) * CMI_NION * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(out_temperature, dTo, sizeof(double) * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(out_pair, dp, sizeof(double) * 2 * n,
                    hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

int cmi_gpu_physics_probe(cmi_gpu_engine *e, int32_t kind, int64_t n,
                          const double *in, double *out) {
  static const int in_width[5] = {1, 1, 15, 1, 1};
  static const int out_width[5] = {CMI_NION, CMI_NION, 1, 5, 3 * CMI_NION};
  if (!e || n <= 0 || !in || !out || kind < 0 || kind > 4)
    return fail(CMI_GPU_EINVAL, "physics_probe: bad argument");
  if (kind == 0 && !e->have_xsec)
    return fail(CMI_GPU_ESTATE, "physics_probe: cross sections not set");
  if (kind == 1 && !e->have_recomb)
    return fail(CMI_GPU_ESTATE, "physics_probe: recombination rates not set");
  HIP_TRY(hipSetDevice(e->device));
  const size_t nin = (size_t)n * in_width[kind];
  const size_t nout = (size_t)n * out_width[kind];
  double *d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof(double) * (nin + nout)));
  hipError_t err =
      hipMemcpy(d, in, sizeof(double) * nin, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    physics_probe_kernel<<<(unsigned)((n + 63) / 64), 64, 0, e->stream>>>(
        e->model, kind, n, d, in_width[kind], d + nin, out_width[kind]);
    err = hipGetLastError();
  }
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(out, d + nin, sizeof(double) * nout,
                    hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

int cmi_gpu_get_timing(cmi_gpu_engine *e, int32_t reset, double *shoot_ms,
                       uint64_t *shoot_launches, double *update_ms,
                       uint64_t *update_launches) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  double s = 0., u = 0.;
  for (auto &p : e->shoot_events) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p.start, p.stop));
    s += ms;
  }
  for (auto &p : e->update_events) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p.start, p.stop));
    u += ms;
  }
  if (shoot_ms)
    *shoot_ms = s;
  if (shoot_launches)
    *shoot_launches = e->shoot_events.size();
  if (update_ms)
    *update_ms = u;
  if (update_launches)
    *update_launches = e->update_events.size();
  if (reset) {
    release_events(e, e->shoot_events);
    release_events(e, e->update_events);
    release_events(e, e->kernel_events);
  }
  return CMI_GPU_OK;
}

int cmi_gpu_get_launch_times(cmi_gpu_engine *e, uint64_t capacity,
                             double *ms, uint64_t *packets, uint64_t *count) {
  if (!e || !count)
    return fail(CMI_GPU_EINVAL, "get_launch_times: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *count = e->kernel_events.size();
  for (uint64_t i = 0; i < e->kernel_events.size() && i < capacity; ++i) {
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, e->kernel_events[i].start,
                                e->kernel_events[i].stop));
    if (ms)
      ms[i] = t;
    if (packets)
      packets[i] = e->kernel_events[i].packets;
  }
  return CMI_GPU_OK;
}

int cmi_gpu_get_launch_steps(cmi_gpu_engine *e, uint64_t capacity,
                             uint64_t *steps, uint64_t *count) {
  if (!e || !count)
    return fail(CMI_GPU_EINVAL, "get_launch_steps: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *count = e->kernel_events.size();
  const uint64_t n = *count < capacity ? *count : capacity;
  if (n && steps)
    HIP_TRY(hipMemcpy(steps, e->launch_steps, sizeof(uint64_t) * n,
                      hipMemcpyDeviceToHost));
  return CMI_GPU_OK;
}

int cmi_gpu_get_kernel_timing(cmi_gpu_engine *e, double *kernel_ms,
                              uint64_t *kernel_launches) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  double k = 0.;
  for (auto &p : e->kernel_events) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p.start, p.stop));
    k += ms;
  }
  if (kernel_ms)
    *kernel_ms = k;
  if (kernel_launches)
    *kernel_launches = e->kernel_events.size();
  return CMI_GPU_OK;
}

/* ------------------------------------------ dusty radiative transfer -- */

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
/* rows per dust_probe_kernel launch */
#define CMI_DUST_PROBE_LAUNCH (1ll << 14)

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

/* the views' descriptors and counters go with a camera that is replaced */
static void dust_free_views(cmi_gpu_engine *e) {
  (void)hipFree(e->dust_views_dev);
  (void)hipFree(e->dust_view_counters);
  e->dust_views_dev = nullptr;
  e->dust_view_counters = nullptr;
  e->dust_views.clear();
  e->sky_views.clear();
  e->dust_nviews = 1;
  e->dust_probe_view = 0;
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

int cmi_gpu_set_ccd_image(cmi_gpu_engine *e, double theta, double phi,
                          int32_t nx, int32_t ny, const double *anchor,
                          const double *sides) {
  if (!e || nx <= 0 || ny <= 0 || !anchor || !sides || !(sides[0] > 0.) ||
      !(sides[1] > 0.) || (int64_t)nx * ny > (1ll << 28))
    return fail(CMI_GPU_EINVAL, "set_ccd_image: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  DustDev &d = e->dust;
  dust_put_view(d, dust_make_view(theta, phi, anchor, sides));
  d.res[0] = nx;
  d.res[1] = ny;
  HIP_TRY(hipStreamSynchronize(e->stream));
  /* no launch may see the old image once it is freed, whatever follows */
  e->have_ccd = false;
  (void)hipFree(e->dust_image);
  e->dust_image = nullptr;
  d.image = nullptr;
  dust_free_views(e);
  const size_t bytes = 3 * (size_t)nx * ny * sizeof(double);
  HIP_TRY(hipMalloc(&e->dust_image, bytes));
  d.image = e->dust_image;
  e->dust_camera = DUST_CAMERA_PARALLEL;
  e->sky_camera.image = nullptr;
  e->have_ccd = true;
  dust_cube_mark_stale(e, "the camera was set again");
  return cmi_gpu_reset_image(e);
}

/* the stack, the descriptors and the counters of a camera with several
 * views, allocated before anything of the engine changes: a call that fails
 * here leaves the camera that was selected */
extern "C++" {
namespace {
struct DustViewBuffers {
  double *images = nullptr;
  void *views = nullptr;
  unsigned long long *counters = nullptr;
  ~DustViewBuffers() {
    (void)hipFree(images);
    (void)hipFree(views);
    (void)hipFree(counters);
  }
};
} // namespace
}

static int dust_alloc_views(const char *what, int32_t nviews, size_t npixel,
                            const void *views, size_t view_bytes,
                            DustViewBuffers &b) {
  hipError_t err = hipMalloc(&b.images, (size_t)nviews * 3 * npixel *
                                            sizeof(double));
  if (err == hipSuccess)
    err = hipMalloc(&b.views, (size_t)nviews * view_bytes);
  if (err == hipSuccess)
    err = hipMalloc(&b.counters, (size_t)nviews * CMI_DUST_VIEW_COUNTERS *
                                     CMI_DUST_VIEW_SLOTS *
                                     sizeof(unsigned long long));
  if (err == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return fail(CMI_GPU_ENOMEM, "%s: the stack of %d images of %zu pixels "
                "does not fit into the device's memory", what, (int)nviews,
                npixel);
  }
  HIP_TRY(err);
  HIP_TRY(hipMemcpy(b.views, views, (size_t)nviews * view_bytes,
                    hipMemcpyHostToDevice));
  return CMI_GPU_OK;
}

/* the engine takes the buffers over from b */
static void dust_adopt_views(cmi_gpu_engine *e, int32_t nviews,
                             DustViewBuffers &b) {
  e->have_ccd = false;
  (void)hipFree(e->dust_image);
  dust_free_views(e);
  e->dust_image = b.images;
  e->dust_views_dev = b.views;
  e->dust_view_counters = b.counters;
  b.images = nullptr;
  b.views = nullptr;
  b.counters = nullptr;
  e->dust_nviews = nviews;
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
  HIP_TRY(hipSetDevice(e->device));
  DustViewBuffers b;
  CMI_TRY(dust_alloc_views("set_ccd_images", nviews, (size_t)nx * ny,
                           views.data(), sizeof(DustViewDev), b));
  HIP_TRY(hipStreamSynchronize(e->stream));
  dust_adopt_views(e, nviews, b);
  DustDev &d = e->dust;
  dust_put_view(d, views[0]);
  d.res[0] = nx;
  d.res[1] = ny;
  d.image = e->dust_image;
  e->dust_views = views;
  e->sky_camera.image = nullptr;
  e->dust_camera = DUST_CAMERA_PARALLEL_VIEWS;
  e->have_ccd = true;
  dust_cube_mark_stale(e, "the cameras were set again");
  return cmi_gpu_reset_image(e);
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
  unsigned int *ninvalid = nullptr;
  HIP_TRY(hipMalloc(&ninvalid, sizeof(unsigned int)));
  unsigned int bad = 0;
  std::vector<double> &B = e->cell_source_blocks_host;
  B.assign((size_t)nblock, 0.);
  hipError_t err = hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream);
  if (err == hipSuccess) {
    cell_source_check_kernel<<<grid_blocks(e, ncell, 8), 256, 0, e->stream>>>(
        e->cell_source_cells, ncell, ninvalid);
    err = hipGetLastError();
  }
  if (err == hipSuccess)
    err = hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                         e->stream);
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  (void)hipFree(ninvalid);
  HIP_TRY(err);
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
  if (!e->have_cells)
    return fail(CMI_GPU_ESTATE, "%s: cell data must be set first", what);
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
  if (e->dust_source == DUST_SOURCE_CELLS && e->cell_source_from_cells &&
      e->cell_source_epoch != e->cells_epoch)
    return fail(CMI_GPU_ESTATE, "dust: the cells changed after the line "
                                "source was set; set_cell_source_line again");
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
  uint64_t size = CMI_DUST_FIRST_LAUNCH;
  const uint64_t min_launch =
      dust_several_views(e)
          ? std::max<uint64_t>(CMI_DUST_MIN_LAUNCH,
                               CMI_DUST_VIEWS_FILLS * (uint64_t)e->num_cu *
                                   CMI_DUST_VIEWS_LANES_PER_CU)
          : CMI_DUST_MIN_LAUNCH;
  for (uint64_t done = 0; done < n;) {
    const uint64_t chunk = std::min<uint64_t>(n - done, size);
    /* only a launch that another follows is measured: both copies are
     * waited for below, before these variables end */
    const bool measure = done + chunk < n;
    unsigned long long steps_before = 0, steps_after = 0;
    if (measure)
      HIP_TRY(hipMemcpyAsync(&steps_before, &e->dust_counters->nsteps,
                             sizeof steps_before, hipMemcpyDeviceToHost,
                             e->stream));
    EventPair ev;
    CMI_TRY(timer_begin(e, ev));
    const unsigned blocks = (unsigned)((chunk + 255) / 256);
    const DustCube<false> no_cube;
    if (e->dust_cube.nchan) {
      /* cube mode: the cube instantiation of the selected camera (the cell
       * source is selected, cmi_gpu_set_scattered_cube and dust_prepare saw
       * to it) */
      const DustCubeDev cube = e->dust_cube;
      if (e->dust_camera == DUST_CAMERA_POINT_VIEWS) {
        DustCamera<DUST_CAMERA_POINT_VIEWS> cam;
        cam.shared = e->sky_camera;
        cam.views = (const SkyObserverDev *)e->dust_views_dev;
        cam.nviews = e->dust_nviews;
        cam.images = e->dust_image;
        cam.counters = e->dust_view_counters;
        dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_POINT_VIEWS, true>
            <<<blocks, 256, 0, e->stream>>>(
                e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
                chunk, e->dust_counters, e->cell_source, cam, cube);
      } else if (e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS) {
        DustCamera<DUST_CAMERA_PARALLEL_VIEWS> cam;
        cam.views = (const DustViewDev *)e->dust_views_dev;
        cam.nviews = e->dust_nviews;
        cam.images = e->dust_image;
        cam.counters = e->dust_view_counters;
        dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_PARALLEL_VIEWS, true>
            <<<blocks, 256, 0, e->stream>>>(
                e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
                chunk, e->dust_counters, e->cell_source, cam, cube);
      } else if (e->dust_camera == DUST_CAMERA_POINT)
        dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_POINT, true>
            <<<blocks, 256, 0, e->stream>>>(
                e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
                chunk, e->dust_counters, e->cell_source, e->sky_camera, cube);
      else
        dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_PARALLEL, true>
            <<<blocks, 256, 0, e->stream>>>(
                e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
                chunk, e->dust_counters, e->cell_source,
                DustCamera<DUST_CAMERA_PARALLEL>(), cube);
    } else if (e->dust_camera == DUST_CAMERA_POINT_VIEWS) {
      DustCamera<DUST_CAMERA_POINT_VIEWS> cam;
      cam.shared = e->sky_camera;
      cam.views = (const SkyObserverDev *)e->dust_views_dev;
      cam.nviews = e->dust_nviews;
      cam.images = e->dust_image;
      cam.counters = e->dust_view_counters;
      dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_POINT_VIEWS, false>
          <<<blocks, 256, 0, e->stream>>>(
              e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
              chunk, e->dust_counters, e->cell_source, cam, no_cube);
    } else if (e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS) {
      DustCamera<DUST_CAMERA_PARALLEL_VIEWS> cam;
      cam.views = (const DustViewDev *)e->dust_views_dev;
      cam.nviews = e->dust_nviews;
      cam.images = e->dust_image;
      cam.counters = e->dust_view_counters;
      if (e->dust_source == DUST_SOURCE_CELLS)
        dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_PARALLEL_VIEWS, false>
            <<<blocks, 256, 0, e->stream>>>(
                e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
                chunk, e->dust_counters, e->cell_source, cam, no_cube);
      else
        dust_shoot_kernel<DUST_SOURCE_GALAXY, DUST_CAMERA_PARALLEL_VIEWS, false>
            <<<blocks, 256, 0, e->stream>>>(
                e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
                chunk, e->dust_counters, DustSource<DUST_SOURCE_GALAXY>(),
                cam, no_cube);
    } else if (e->dust_camera == DUST_CAMERA_POINT)
      dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_POINT, false>
          <<<blocks, 256, 0, e->stream>>>(
              e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
              chunk, e->dust_counters, e->cell_source, e->sky_camera,
              no_cube);
    else if (e->dust_source == DUST_SOURCE_CELLS)
      dust_shoot_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_PARALLEL, false>
          <<<blocks, 256, 0, e->stream>>>(
              e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
              chunk, e->dust_counters, e->cell_source,
              DustCamera<DUST_CAMERA_PARALLEL>(), no_cube);
    else
      dust_shoot_kernel<DUST_SOURCE_GALAXY, DUST_CAMERA_PARALLEL, false>
          <<<blocks, 256, 0, e->stream>>>(
              e->grid, e->dust, e->dust_opacity, seed, first_packet + done,
              chunk, e->dust_counters, DustSource<DUST_SOURCE_GALAXY>(),
              DustCamera<DUST_CAMERA_PARALLEL>(), no_cube);
    HIP_TRY(hipGetLastError());
    CMI_TRY(timer_end(e, e->shoot_events, ev, chunk));
    done += chunk;
    if (measure) {
      /* the next launch's size from this one's steps per packet */
      HIP_TRY(hipMemcpyAsync(&steps_after, &e->dust_counters->nsteps,
                             sizeof steps_after, hipMemcpyDeviceToHost,
                             e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      const double per_packet =
          std::max(1., (double)(steps_after - steps_before) / (double)chunk);
      size = (uint64_t)std::min<double>(
          (double)CMI_DUST_MAX_LAUNCH,
          std::max<double>((double)min_launch,
                           (double)CMI_DUST_STEPS_PER_LAUNCH / per_packet));
    }
  }
  return CMI_GPU_OK;
}

int cmi_gpu_get_dust_counters(cmi_gpu_engine *e, uint64_t *counters) {
  if (!e || !counters)
    return fail(CMI_GPU_EINVAL, "get_dust_counters: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  DustCountersDev c = {};
  if (e->dust_counters)
    HIP_TRY(hipMemcpy(&c, e->dust_counters, sizeof c, hipMemcpyDeviceToHost));
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
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  DustCountersDev c = {};
  if (e->dust_counters)
    HIP_TRY(hipMemcpy(&c, e->dust_counters, sizeof c, hipMemcpyDeviceToHost));
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
  if (view < 0 || view >= e->dust_nviews)
    return fail(CMI_GPU_EINVAL, "download_image_view: view %d of %d",
                (int)view, (int)e->dust_nviews);
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
  if (view < 0 || view >= e->dust_nviews)
    return fail(CMI_GPU_EINVAL, "get_dust_view_counters: view %d of %d",
                (int)view, (int)e->dust_nviews);
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
  if (view < 0 || view >= e->dust_nviews)
    return fail(CMI_GPU_EINVAL, "select_probe_view: view %d of %d", (int)view,
                (int)e->dust_nviews);
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
  double *din = nullptr, *dout = nullptr;
  const size_t in_bytes = (size_t)n * in_width[kind] * sizeof(double);
  const size_t out_bytes = (size_t)n * width * sizeof(double);
  HIP_TRY(hipMalloc(&dout, out_bytes));
  hipError_t err = hipSuccess;
  if (in_bytes) {
    err = hipMalloc(&din, in_bytes);
    if (err == hipSuccess)
      err = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice);
  }
  if (err == hipSuccess)
    err = hipMemsetAsync(dout, 0, out_bytes, e->stream);
  /* short launches: a row of a trace can be a whole packet */
  for (int64_t k = 0; err == hipSuccess && k < n; k += CMI_DUST_PROBE_LAUNCH) {
    const int64_t m = std::min<int64_t>(n - k, CMI_DUST_PROBE_LAUNCH);
    const unsigned blocks = (unsigned)((m + 63) / 64);
    const double *rows = din ? din + k * in_width[kind] : nullptr;
    const DustCube<false> no_cube;
    if (kind == DUST_PROBE_CUBE_TRACE && dust_point_camera(e))
      dust_probe_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_POINT, true>
          <<<blocks, 64, 0, e->stream>>>(
              e->grid, dust, e->cell_source, sky_camera, cube,
              e->dust_opacity, kind, seed, first_packet + k, m, width, rows,
              dout + k * width, max_events);
    else if (kind == DUST_PROBE_CUBE_TRACE)
      dust_probe_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_PARALLEL, true>
          <<<blocks, 64, 0, e->stream>>>(
              e->grid, dust, e->cell_source,
              DustCamera<DUST_CAMERA_PARALLEL>(), cube, e->dust_opacity, kind,
              seed, first_packet + k, m, width, rows, dout + k * width,
              max_events);
    else if (dust_point_camera(e))
      dust_probe_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_POINT, false>
          <<<blocks, 64, 0, e->stream>>>(
              e->grid, dust, e->cell_source, sky_camera, no_cube,
              e->dust_opacity, kind, seed, first_packet + k, m, width, rows,
              dout + k * width, max_events);
    else if (e->dust_source == DUST_SOURCE_CELLS)
      dust_probe_kernel<DUST_SOURCE_CELLS, DUST_CAMERA_PARALLEL, false>
          <<<blocks, 64, 0, e->stream>>>(
              e->grid, dust, e->cell_source,
              DustCamera<DUST_CAMERA_PARALLEL>(), no_cube, e->dust_opacity,
              kind, seed, first_packet + k, m, width, rows, dout + k * width,
              max_events);
    else
      dust_probe_kernel<DUST_SOURCE_GALAXY, DUST_CAMERA_PARALLEL, false>
          <<<blocks, 64, 0, e->stream>>>(
              e->grid, dust, DustSource<DUST_SOURCE_GALAXY>(),
              DustCamera<DUST_CAMERA_PARALLEL>(), no_cube, e->dust_opacity,
              kind, seed, first_packet + k, m, width, rows, dout + k * width,
              max_events);
    err = hipGetLastError();
    if (err == hipSuccess)
      err = hipStreamSynchronize(e->stream);
  }
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

/* the ray-traced renderers: line images and cubes, sky maps and cubes, the
 * radio continuum */
#include "render_driver.h"

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
  HIP_TRY(hipSetDevice(e->device));
  SkyCameraDev cam = {};
  sky_put_observer(cam, sky_make_observer(origin, frame, exclusion_radius));
  cam.lon_min = lon_min;
  cam.lat_min = lat_min;
  cam.lon_width = lon_max - lon_min;
  cam.lat_width = lat_max - lat_min;
  cam.nlon = nlon;
  cam.nlat = nlat;
  cam.direct_light = direct_light != 0;
  HIP_TRY(hipStreamSynchronize(e->stream));
  /* no launch may see the old image once it is freed, whatever follows */
  e->have_ccd = false;
  (void)hipFree(e->dust_image);
  e->dust_image = nullptr;
  dust_free_views(e);
  e->dust.image = nullptr;
  e->sky_camera.image = nullptr;
  HIP_TRY(hipMalloc(&e->dust_image,
                    3 * (size_t)nlon * nlat * sizeof(double)));
  cam.image = e->dust_image;
  e->sky_camera = cam;
  e->dust_camera = DUST_CAMERA_POINT;
  e->have_ccd = true;
  dust_cube_mark_stale(e, "the camera was set again");
  return cmi_gpu_reset_image(e);
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
  HIP_TRY(hipSetDevice(e->device));
  DustViewBuffers b;
  CMI_TRY(dust_alloc_views("set_sky_cameras", nviews, (size_t)nlon * nlat,
                           views.data(), sizeof(SkyObserverDev), b));
  HIP_TRY(hipStreamSynchronize(e->stream));
  dust_adopt_views(e, nviews, b);
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
  e->sky_views = views;
  e->dust.image = nullptr;
  e->dust_camera = DUST_CAMERA_POINT_VIEWS;
  e->have_ccd = true;
  dust_cube_mark_stale(e, "the cameras were set again");
  return cmi_gpu_reset_image(e);
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
  if (!e->have_ccd)
    return fail(CMI_GPU_ESTATE, "%s: a camera must be set first", what);
  if (e->dust_source != DUST_SOURCE_CELLS || !e->have_cell_source)
    return fail(CMI_GPU_ESTATE, "%s: a cell source must be selected (the "
                "spiral galaxy has no line)", what);
  const bool line = e->cell_source_from_cells;
  if (line && e->cell_source_epoch != e->cells_epoch)
    return fail(CMI_GPU_ESTATE, "%s: the cells changed after the line source "
                "was set; set_cell_source_line again", what);
  if (line && widths)
    return fail(CMI_GPU_ESTATE, "%s: a line source takes its widths from the "
                "cells' temperatures; widths must be NULL", what);
  if (!line && !widths)
    return fail(CMI_GPU_ESTATE, "%s: a field source needs widths[ncell]",
                what);
  if (line && cmi_emission_atomic_weight[e->cell_source_line] == 0.)
    return fail(CMI_GPU_EINVAL, "%s: entry %d is not the line of one ion: it "
                "has no line profile", what, (int)e->cell_source_line);
  if (!(sigma_turb >= 0.) || !std::isfinite(sigma_turb))
    return fail(CMI_GPU_EINVAL, "%s: the turbulent velocity dispersion must "
                "be >= 0 and finite", what);
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
  const size_t ncell = (size_t)e->ncell;
  /* everything new is built aside: a call that fails leaves the previous
   * state in place */
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  double *s2 = nullptr, *vobs = nullptr, *cube = nullptr, *dwidths = nullptr;
  unsigned int *ninvalid = nullptr;
  unsigned int bad = 0;
  std::vector<double> vo(3 * (size_t)nviews, 0.);
  if (observer_velocities)
    std::copy(observer_velocities, observer_velocities + vo.size(),
              vo.begin());
  hipError_t err = hipMalloc(&s2, sizeof(double) * ncell);
  if (err == hipSuccess)
    err = hipMalloc(&vobs, sizeof(double) * vo.size());
  if (err == hipSuccess)
    err = hipMalloc(&cube, sizeof(double) * 3 * (size_t)nviews * npixel * nchan);
  if (err == hipSuccess)
    err = hipMemcpy(vobs, vo.data(), sizeof(double) * vo.size(),
                    hipMemcpyHostToDevice);
  if (err == hipSuccess && line) {
    dust_cube_line_variance_kernel<<<(unsigned)((ncell + 255) / 256), 256, 0,
                                     e->stream>>>(
        cells->temperature, cmi_emission_atomic_weight[e->cell_source_line],
        sigma_turb, e->ncell, s2);
    err = hipGetLastError();
  } else if (err == hipSuccess) {
    err = hipMalloc(&dwidths, sizeof(double) * ncell);
    if (err == hipSuccess)
      err = hipMalloc(&ninvalid, sizeof(unsigned int));
    if (err == hipSuccess)
      err = hipMemcpy(dwidths, widths, sizeof(double) * ncell,
                      hipMemcpyHostToDevice);
    if (err == hipSuccess)
      err = hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream);
    if (err == hipSuccess) {
      dust_cube_field_variance_kernel<<<grid_blocks(e, e->ncell, 8), 256, 0,
                                        e->stream>>>(dwidths, e->ncell, s2,
                                                     ninvalid);
      err = hipGetLastError();
    }
    if (err == hipSuccess)
      err = hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                           e->stream);
  }
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  (void)hipFree(dwidths);
  (void)hipFree(ninvalid);
  int rc = CMI_GPU_OK;
  if (err == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    rc = fail(CMI_GPU_ENOMEM, "%s: %d cubes of %d channels of %zu pixels do "
              "not fit into the device's memory", what, (int)nviews,
              (int)nchan, npixel);
  } else if (err != hipSuccess) {
    rc = fail(CMI_GPU_EDEVICE, "%s: %s", what, hipGetErrorString(err));
  } else if (bad) {
    rc = fail(CMI_GPU_EINVAL, "%s: %u width(s) are negative or not finite",
              what, bad);
  }
  if (rc) {
    (void)hipFree(s2);
    (void)hipFree(vobs);
    (void)hipFree(cube);
    return rc;
  }
  dust_cube_free(e);
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
  double *ordered = nullptr;
  HIP_TRY(hipMalloc(&ordered, sizeof(double) * nvalue));
  double *dst[3] = {I, Q, U};
  hipError_t err = hipSuccess;
  for (int k = 0; k < 3 && err == hipSuccess; ++k) {
    if (!dst[k])
      continue;
    dust_cube_reorder_kernel<<<(unsigned)((nvalue + 255) / 256), 256, 0,
                               e->stream>>>(
        c.cube + (3 * (size_t)view + k) * nvalue, c.npixel, c.nchan, ordered);
    err = hipGetLastError();
    if (err == hipSuccess)
      err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess)
      err = hipMemcpy(dst[k], ordered, sizeof(double) * nvalue,
                      hipMemcpyDeviceToHost);
  }
  (void)hipFree(ordered);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

/* ------------------------------------------------------- Lyman alpha -- */

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
  if (!e->have_cells)
    return fail(CMI_GPU_ESTATE, "%s: cell data must be set first", what);
  if (!e->have_ccd)
    return fail(CMI_GPU_ESTATE, "%s: a camera must be set first", what);
  if (dust_point_camera(e))
    return fail(CMI_GPU_ESTATE, "%s: the point (sky) cameras are not "
                "supported; set_ccd_image or set_ccd_images", what);
  if (e->dust_source != DUST_SOURCE_CELLS || !e->have_cell_source)
    return fail(CMI_GPU_ESTATE, "%s: a cell source must be selected "
                "(set_cell_source_field or set_cell_source_line)", what);
  if (e->cell_source_from_cells && e->cell_source_epoch != e->cells_epoch)
    return fail(CMI_GPU_ESTATE, "%s: the cells changed after the line source "
                "was set; set_cell_source_line again", what);
  if (e->have_dust_scattering && !e->dust_per_hydrogen)
    return fail(CMI_GPU_ESTATE, "%s: the dust must be given per hydrogen "
                "nucleus (set_dust_scattering_per_hydrogen)", what);
  if (!(sigma_turb >= 0.) || !std::isfinite(sigma_turb))
    return fail(CMI_GPU_EINVAL, "%s: the turbulent velocity dispersion must "
                "be >= 0 and finite", what);
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
  const size_t ncell = (size_t)e->ncell;
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  /* everything new is built aside: a call that fails leaves the previous
   * state in place */
  LyaRecord *records = nullptr;
  double *image = nullptr, *cube = nullptr, *dn = nullptr, *dT = nullptr;
  unsigned int *ninvalid = nullptr;
  unsigned int bad = 0;
  hipError_t err = hipMalloc(&records, sizeof(LyaRecord) * ncell);
  if (err == hipSuccess)
    err = hipMalloc(&image, sizeof(double) * (size_t)nviews * npixel);
  if (err == hipSuccess)
    err = hipMalloc(&cube, sizeof(double) * (size_t)nviews * npixel * nchan);
  if (err == hipSuccess)
    err = hipMalloc(&ninvalid, sizeof(unsigned int));
  if (err == hipSuccess && n_HI) {
    err = hipMalloc(&dn, sizeof(double) * ncell);
    if (err == hipSuccess)
      err = hipMemcpy(dn, n_HI, sizeof(double) * ncell, hipMemcpyHostToDevice);
  }
  if (err == hipSuccess && temperature) {
    err = hipMalloc(&dT, sizeof(double) * ncell);
    if (err == hipSuccess)
      err = hipMemcpy(dT, temperature, sizeof(double) * ncell,
                      hipMemcpyHostToDevice);
  }
  if (err == hipSuccess && !e->lya_next)
    err = hipMalloc(&e->lya_next, sizeof(unsigned long long));
  if (err == hipSuccess && !e->lya_counters)
    err = hipMalloc(&e->lya_counters, sizeof(LyaCountersDev));
  if (err == hipSuccess)
    err = hipMemsetAsync(ninvalid, 0, sizeof(unsigned int), e->stream);
  if (err == hipSuccess) {
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
    err = hipGetLastError();
  }
  if (err == hipSuccess)
    err = hipMemcpyAsync(&bad, ninvalid, sizeof bad, hipMemcpyDeviceToHost,
                         e->stream);
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  (void)hipFree(dn);
  (void)hipFree(dT);
  (void)hipFree(ninvalid);
  int rc = CMI_GPU_OK;
  if (err == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    rc = fail(CMI_GPU_ENOMEM, "%s: %d cubes of %d channels of %zu pixels do "
              "not fit into the device's memory", what, (int)nviews,
              (int)nchan, npixel);
  } else if (err != hipSuccess) {
    rc = fail(CMI_GPU_EDEVICE, "%s: %s", what, hipGetErrorString(err));
  } else if (bad) {
    rc = fail(CMI_GPU_EINVAL, "%s: %u cell(s) have a Doppler width that is not "
              "positive and finite (T and sigma_turb both 0?) or a density "
              "that is negative or not finite", what, bad);
  }
  if (rc) {
    (void)hipFree(records);
    (void)hipFree(image);
    (void)hipFree(cube);
    return rc;
  }
  lya_free(e);
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
  if (!e->lya.nchan)
    return fail(CMI_GPU_ESTATE, "%s: Lyman-alpha mode is not set "
                "(set_lyman_alpha)", what);
  if (e->lya_stale)
    return fail(CMI_GPU_ESTATE, "%s: %s after Lyman-alpha mode was set; "
                "set_lyman_alpha again", what, e->lya_stale);
  if (e->cell_source_from_cells && e->cell_source_epoch != e->cells_epoch)
    return fail(CMI_GPU_ESTATE, "%s: the cells changed after the line source "
                "was set; set_cell_source_line again", what);
  HIP_TRY(hipSetDevice(e->device));
  dust = e->lya_dust;
  return CMI_GPU_OK;
}

static DustCamera<DUST_CAMERA_PARALLEL_VIEWS> lya_views(cmi_gpu_engine *e) {
  DustCamera<DUST_CAMERA_PARALLEL_VIEWS> cam;
  cam.views = (const DustViewDev *)e->dust_views_dev;
  cam.nviews = e->dust_nviews;
  cam.images = e->dust_image;
  cam.counters = e->dust_view_counters;
  return cam;
}

int cmi_gpu_lya_shoot(cmi_gpu_engine *e, uint32_t seed, uint64_t first_packet,
                      uint64_t n) {
  DustDev dust;
  CMI_TRY(lya_prepare(e, "lya_shoot", dust));
  uint64_t size = CMI_LYA_FIRST_LAUNCH;
  for (uint64_t done = 0; done < n;) {
    const uint64_t chunk = std::min<uint64_t>(n - done, size);
    const bool measure = done + chunk < n;
    unsigned long long steps_before = 0, steps_after = 0;
    if (measure)
      HIP_TRY(hipMemcpyAsync(&steps_before, &e->lya_counters->nsteps,
                             sizeof steps_before, hipMemcpyDeviceToHost,
                             e->stream));
    HIP_TRY(hipMemsetAsync(e->lya_next, 0, sizeof(unsigned long long),
                           e->stream));
    EventPair ev;
    CMI_TRY(timer_begin(e, ev));
#ifndef CMI_LYA_EVENT_LOOP
    const unsigned blocks = (unsigned)((chunk + 255) / 256);
#else
    const unsigned blocks = (unsigned)std::min<uint64_t>(
        (chunk + 255) / 256, (uint64_t)e->num_cu * CMI_LYA_BLOCKS_PER_CU);
#endif
    /* the field's launches are instantiations of their own: without it the
     * kernels are the ones they were */
    const LyaFieldDev field = {e->lya_field, 1. - dust.albedo * dust.hgg};
    if (e->lya_field && e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS)
      lya_shoot_kernel<DUST_CAMERA_PARALLEL_VIEWS, LyaFieldDev>
          <<<blocks, 256, 0, e->stream>>>(
              e->grid, dust, e->cell_source, lya_views(e), e->lya, seed,
              first_packet + done, chunk, e->lya_next, e->lya_counters, field);
    else if (e->lya_field)
      lya_shoot_kernel<DUST_CAMERA_PARALLEL, LyaFieldDev>
          <<<blocks, 256, 0, e->stream>>>(
              e->grid, dust, e->cell_source,
              DustCamera<DUST_CAMERA_PARALLEL>(), e->lya, seed,
              first_packet + done, chunk, e->lya_next, e->lya_counters, field);
    else if (e->dust_camera == DUST_CAMERA_PARALLEL_VIEWS)
      lya_shoot_kernel<DUST_CAMERA_PARALLEL_VIEWS>
          <<<blocks, 256, 0, e->stream>>>(
              e->grid, dust, e->cell_source, lya_views(e), e->lya, seed,
              first_packet + done, chunk, e->lya_next, e->lya_counters);
    else
      lya_shoot_kernel<DUST_CAMERA_PARALLEL><<<blocks, 256, 0, e->stream>>>(
          e->grid, dust, e->cell_source, DustCamera<DUST_CAMERA_PARALLEL>(),
          e->lya, seed, first_packet + done, chunk, e->lya_next,
          e->lya_counters);
    HIP_TRY(hipGetLastError());
    CMI_TRY(timer_end(e, e->shoot_events, ev, chunk));
    done += chunk;
    if (measure) {
      HIP_TRY(hipMemcpyAsync(&steps_after, &e->lya_counters->nsteps,
                             sizeof steps_after, hipMemcpyDeviceToHost,
                             e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      const double per_packet =
          std::max(1., (double)(steps_after - steps_before) / (double)chunk);
      size = (uint64_t)std::min<double>(
          (double)CMI_LYA_MAX_LAUNCH,
          std::max<double>((double)CMI_LYA_MIN_LAUNCH,
                           (double)CMI_LYA_STEPS_PER_LAUNCH / per_packet));
    }
  }
  return CMI_GPU_OK;
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
  if (!e->lya.nchan)
    return fail(CMI_GPU_ESTATE, "%s: Lyman-alpha mode is not set "
                "(set_lyman_alpha)", what);
  if (e->lya_stale)
    return fail(CMI_GPU_ESTATE, "%s: %s after Lyman-alpha mode was set", what,
                e->lya_stale);
  if (view < 0 || view >= e->lya_nviews)
    return fail(CMI_GPU_EINVAL, "%s: view %d of %d", what, (int)view,
                (int)e->lya_nviews);
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
  double *ordered = nullptr;
  HIP_TRY(hipMalloc(&ordered, sizeof(double) * nvalue));
  dust_cube_reorder_kernel<<<(unsigned)((nvalue + 255) / 256), 256, 0,
                             e->stream>>>(l.cube + (size_t)view * nvalue,
                                          l.npixel, l.nchan, ordered);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(cube, ordered, sizeof(double) * nvalue,
                    hipMemcpyDeviceToHost);
  (void)hipFree(ordered);
  HIP_TRY(err);
  return CMI_GPU_OK;
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
  double *din = nullptr, *dout = nullptr;
  const size_t in_bytes = (size_t)n * in_width[kind] * sizeof(double);
  const size_t out_bytes = (size_t)n * width * sizeof(double);
  HIP_TRY(hipMalloc(&dout, out_bytes));
  hipError_t err = hipSuccess;
  if (in_bytes) {
    err = hipMalloc(&din, in_bytes);
    if (err == hipSuccess)
      err = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice);
  }
  if (err == hipSuccess)
    err = hipMemsetAsync(dout, 0, out_bytes, e->stream);
  for (int64_t k = 0; err == hipSuccess && k < n; k += CMI_DUST_PROBE_LAUNCH) {
    const int64_t m = std::min<int64_t>(n - k, CMI_DUST_PROBE_LAUNCH);
    lya_probe_kernel<DUST_CAMERA_PARALLEL>
        <<<(unsigned)((m + 63) / 64), 64, 0, e->stream>>>(
            e->grid, dust, e->cell_source, DustCamera<DUST_CAMERA_PARALLEL>(),
            e->lya, kind, seed, first_packet + k, m, width,
            din ? din + k * in_width[kind] : nullptr, dout + k * width,
            max_events);
    err = hipGetLastError();
    if (err == hipSuccess)
      err = hipStreamSynchronize(e->stream);
  }
  if (err == hipSuccess)
    err = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

int cmi_gpu_set_lya_field(cmi_gpu_engine *e, int32_t enable) {
  static const char *what = "set_lya_field";
  if (!e)
    return fail(CMI_GPU_EINVAL, "%s: null engine", what);
  if (!e->lya.nchan)
    return fail(CMI_GPU_ESTATE, "%s: Lyman-alpha mode is not set "
                "(set_lyman_alpha)", what);
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
  if (!e->lya.nchan)
    return fail(CMI_GPU_ESTATE, "%s: Lyman-alpha mode is not set "
                "(set_lyman_alpha)", what);
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
  double *out = nullptr;
  HIP_TRY(hipMalloc(&out, sizeof(double) * 2 * ncell));
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
  hipError_t err = hipGetLastError();
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess && P_alpha)
    err = hipMemcpy(P_alpha, out, sizeof(double) * ncell,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(T_s, out + ncell, sizeof(double) * ncell,
                    hipMemcpyDeviceToHost);
  (void)hipFree(out);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

int cmi_gpu_lyman_alpha_emissivity(cmi_gpu_engine *e, double *out) {
  static const char *what = "lyman_alpha_emissivity";
  if (!e || !out)
    return fail(CMI_GPU_EINVAL, "%s: null argument", what);
  if (!e->have_cells)
    return fail(CMI_GPU_ESTATE, "%s: cell data must be set first", what);
  HIP_TRY(hipSetDevice(e->device));
  CellsDev *cells;
  CMI_TRY(cells_settled(e, cells));
  double *dev = nullptr;
  HIP_TRY(hipMalloc(&dev, sizeof(double) * (size_t)e->ncell));
  lya_emissivity_kernel<<<(unsigned)((e->ncell + 255) / 256), 256, 0,
                          e->stream>>>(
      cells->number_density, cells->temperature, cells->x[0], cells->x[1],
      e->model.abundance[0], e->ncell, dev);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess)
    err = hipMemcpy(out, dev, sizeof(double) * (size_t)e->ncell,
                    hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  HIP_TRY(err);
  return CMI_GPU_OK;
}

} // extern "C"

#include "group.h"
