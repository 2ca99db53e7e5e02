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
#include "absorption_kernels.h"
#include "sph_map_kernels.h"
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
  /* 32-bit words of the block the keys and ids live in: 4 per packet, or
   * what the bucket order lays into it (BucketPlan::total_words) */
  uint64_t sort_block_words = 0;
  /* the bucket order's cursors, leaf offsets and counts (bucket_meta_words) */
  uint32_t *bucket_meta = nullptr;
  /* how the last launch of new packets was ordered (OrderPath), the bits of
   * its two scatter levels: cmi_gpu_get_order_plan */
  int32_t last_order_path = 0;
  int32_t last_bucket_bits[2] = {0, 0};
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
  /* the escape tally (cmi_gpu_set_escape_tally); counted like a tracker */
  EscapeDev escape = {};
  /* its copy behind the counters (cmi_escape_of) holds the array's address
   * (publish_escape); what that copy was written from */
  bool escape_counting = false;
  EscapeDev escape_staged = {};
  /* what the last SPH mapping did (cmi_gpu_get_sph_map_stats) */
  int64_t sph_map_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  /* PAD transport kernels: sigma_H n x_H inside a layer of ghost cells;
   * whether it holds the records of the cells and the cross section as they
   * are (whatever writes CellsDev::opacity clears this - pad_records_stale -
   * except the update that writes the padded records itself,
   * hydrogen_update_kernel; so does every setter of the cross sections,
   * update_full_flag) */
  double *pad_H = nullptr;
  bool pad_valid = false;
  /* the first-generation build of the last transport call's plan (FirstBuild)
   * and whether it was the UNIFORM one: cmi_gpu_get_transport_plan */
  int32_t last_first_build = 0;
  bool last_pad_uniform = false;
  /* ... and whether it was the bundle build: cmi_gpu_get_bundle_march */
  bool last_bundle_march = false;
  /* ... and the point build of it: cmi_gpu_get_bundle_point */
  bool last_bundle_point = false;
  /* the block that build's refill reads, written ahead of every launch of it
   * (write_point_block) */
  PointEmitDev *point_emit = nullptr;
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
    /* the coarse direction bins of that key hold this many chunks of 64 per
     * tau class (key_args): with 8 a (bin, class) group is wider than a span,
     * so the chunks a block's waves fly in one round come from one class or
     * two neighbouring ones */
    int class_group_chunks = 1;
    /* hydrogen-only launches of bucket_min_packets packets and more: ordered
     * by two scatter levels and a sort of the leaves in LDS (packet_order.h)
     * instead of the radix sort; the levels' bits and the room of a region
     * and a leaf beyond its mean, in thousandths (-1: packet_order_plan.h
     * chooses) */
    bool bucket_order = true;
    int bucket_bits1 = -1, bucket_bits2 = -1;
    int bucket_slack_permille = -1;
    uint64_t bucket_min_packets = 1000000;
    int aggregate = CMI_AGG_BLOCK;     /* first generation (sorted bundles) */
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
    /* ... and, where every packet of a call carries one weight and no heating
     * term is tracked, sum path lengths and weigh the sums at the flush
     * (shoot_kernel<..., PAD, UNIFORM>) */
    bool pad_uniform = true;
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
    /* the padded first generation whose every refill fills a whole idle wave
     * (chunk 64, refill_threshold 64, claimed spans, new packets, no heating,
     * no re-emission, an undivided grid): the bundle build,
     * shoot_bundle_kernel (false: the general kernel) */
    bool bundle_march = true;
    /* ... and, where all its packets come from one discrete source and no
     * continuous one, the point build of that kernel
     * (shoot_bundle_kernel<true, true>; false: the bundle build) */
    bool bundle_point = true;
    bool phase_stamps = false; /* experiments build: ShootArgs::phase_clock */
    /* continuum images: channels per march launch (4, 8 or 16) and the rays
     * per launch (0: the images' and the sky maps' own bounds) */
    int continuum_channel_block = CMI_CONTINUUM_FB;
    int64_t continuum_launch_rays = 0;
    int absorbing_cube_channel_block = CMI_ABSORBING_CB;
    int absorbing_cube_expm1_call = CMI_ABSORBING_EXPM1_CALL;
    int absorbing_cube_window_skip = 1;
    int64_t absorbing_cube_launch_rays = 0;
    /* absorption spectra: slab rows per wave (1, 2 or 4; 0: by the number of
     * channels, CMI_ABSORPTION_R at most), the upper edge's E
     * from the neighbouring lane, the two exact skips */
    int absorption_slab_rows = 0;
    int absorption_edge_sharing = CMI_ABSORPTION_EDGE_SHARING;
    int absorption_skips = 1;
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
  /* (every setter of the cross sections ends here: the padded records hold
   * sigma_H n x_H - cmi_pad_record - and are those of another model now) */
  e->pad_valid = false;
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
  /* (... and the escape tally's description behind them, cmi_escape_of) */
  HIP_TRY(hipMalloc(&e->counters, sizeof(CountersDev) * CMI_COUNTER_SHARDS +
                                      sizeof(EscapeDev)));
  HIP_TRY(hipMemsetAsync(e->counters, 0,
                         sizeof(CountersDev) * CMI_COUNTER_SHARDS +
                             sizeof(EscapeDev),
                         e->stream));
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
  (void)hipFree(e->escape.sky);
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
  (void)hipFree(e->point_emit);
#ifdef CMI_EXPERIMENTS
  (void)hipFree(e->phase_clock);
#endif
  (void)hipFree(e->select_ids);
  (void)hipFree(e->select_rows);
  (void)hipFree(e->sort_temp);
  (void)hipFree(e->bucket_meta);
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

int cmi_gpu_get_transport_plan(cmi_gpu_engine *e, int32_t *first_build,
                               int32_t *uniform_weight) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (first_build)
    *first_build = e->last_first_build;
  if (uniform_weight)
    *uniform_weight = e->last_pad_uniform ? 1 : 0;
  return CMI_GPU_OK;
}

int cmi_gpu_get_bundle_march(cmi_gpu_engine *e, int32_t *flown) {
  if (!e || !flown)
    return fail(CMI_GPU_EINVAL, "get_bundle_march: bad argument");
  *flown = e->last_bundle_march ? 1 : 0;
  return CMI_GPU_OK;
}

int cmi_gpu_get_bundle_point(cmi_gpu_engine *e, int32_t *flown) {
  if (!e || !flown)
    return fail(CMI_GPU_EINVAL, "get_bundle_point: bad argument");
  *flown = e->last_bundle_point ? 1 : 0;
  return CMI_GPU_OK;
}

/* the words of cmi_gpu_engine::bucket_meta: the regions' and the leaves'
 * cursors, the overflow list's, the count of ordered ids - cleared before
 * every launch - and the leaves' offsets */
#define CMI_BUCKET_META_LEAF_CURSOR                                            \
  ((size_t)CMI_BUCKET_MAX * CMI_BUCKET_REGION_CURSOR_STRIDE)
#define CMI_BUCKET_META_OVERFLOW                                               \
  (CMI_BUCKET_META_LEAF_CURSOR + (size_t)CMI_BUCKET_MAX * CMI_BUCKET_MAX)
#define CMI_BUCKET_META_ORDERED (CMI_BUCKET_META_OVERFLOW + 1)
#define CMI_BUCKET_META_CLEARED (CMI_BUCKET_META_OVERFLOW + 8)
#define CMI_BUCKET_META_LEAF_OFFSET CMI_BUCKET_META_CLEARED
#define CMI_BUCKET_META_WORDS                                                  \
  (CMI_BUCKET_META_LEAF_OFFSET + (size_t)CMI_BUCKET_MAX * CMI_BUCKET_MAX)
static uint32_t *bucket_overflow_cursor(const cmi_gpu_engine *e) {
  return e->bucket_meta + CMI_BUCKET_META_OVERFLOW;
}

int cmi_gpu_get_order_plan(cmi_gpu_engine *e, int32_t *path, int32_t *bits1,
                           int32_t *bits2, uint64_t *overflow) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  const bool bucket = e->last_order_path == CMI_GPU_ORDER_BUCKET;
  if (path)
    *path = e->last_order_path;
  if (bits1)
    *bits1 = bucket ? e->last_bucket_bits[0] : 0;
  if (bits2)
    *bits2 = bucket ? e->last_bucket_bits[1] : 0;
  if (overflow) {
    *overflow = 0;
    if (bucket) {
      /* (the launch's cursors stay as they are until the next launch) */
      uint32_t sent = 0;
      HIP_TRY(hipSetDevice(e->device));
      HIP_TRY(hipStreamSynchronize(e->stream));
      HIP_TRY(hipMemcpy(&sent, bucket_overflow_cursor(e), sizeof sent,
                        hipMemcpyDeviceToHost));
      *overflow = sent;
    }
  }
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
  else if (k == "class_group_chunks")
    e->tune.class_group_chunks =
        (int)(value < 1 ? 1 : (value > 64 ? 64 : value));
  else if (k == "bucket_order")
    e->tune.bucket_order = value != 0;
  else if (k == "bucket_bits1")
    e->tune.bucket_bits1 = (int)(value < 0 ? -1 : (value > 8 ? 8 : value));
  else if (k == "bucket_bits2")
    e->tune.bucket_bits2 = (int)(value < 0 ? -1 : (value > 8 ? 8 : value));
  else if (k == "bucket_slack_permille")
    e->tune.bucket_slack_permille =
        (int)(value < 0 ? -1 : (value > 1000000 ? 1000000 : value));
  else if (k == "bucket_min_packets")
    e->tune.bucket_min_packets = (uint64_t)(value < 0 ? 0 : value);
  else if (k == "aggregate")
    e->tune.aggregate =(int)(value < 0 ? 0 : (value > 2 ? 2 : value));
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
  else if (k == "pad_uniform")
    e->tune.pad_uniform = value != 0;
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
  else if (k == "bundle_march")
    e->tune.bundle_march = value != 0;
  else if (k == "bundle_point")
    e->tune.bundle_point = value != 0;
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
  else if (k == "absorption_slab_rows") {
    if (value != 0 && value != 1 && value != 2 && value != 4)
      return fail(CMI_GPU_EINVAL, "set_tuning: absorption_slab_rows is 1, 2 "
                  "or 4, or 0 for the default (%lld asked for)",
                  (long long)value);
    e->tune.absorption_slab_rows = (int)value;
  } else if (k == "absorption_edge_sharing")
    e->tune.absorption_edge_sharing = value != 0;
  else if (k == "absorption_skips")
    e->tune.absorption_skips = value != 0;
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

int cmi_gpu_order_packets(cmi_gpu_engine *e, uint32_t seed, uint32_t iteration,
                          uint64_t first_packet, uint64_t n, uint32_t *out_ids,
                          uint32_t *out_keys) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (!e->have_sources || (e->model.nsource > 0 && !e->have_spectrum) ||
      (e->model.continuous_type != 0 && !e->have_continuous_spectrum) ||
      !e->have_xsec || !e->have_cells)
    return fail(CMI_GPU_ESTATE,
                "order_packets: sources, their spectra, cross sections and "
                "cell data must be set first");
  if (n == 0)
    return CMI_GPU_OK;
  if (n > e->tune.max_packets_per_launch)
    return fail(CMI_GPU_EINVAL, "order_packets: %llu packets are more than "
                "one launch (max_packets_per_launch)", (unsigned long long)n);
  HIP_TRY(hipSetDevice(e->device));
  CMI_TRY(ensure_spectra(e));
  LaunchPlan plan;
  CMI_TRY(plan_launches(e, n, nullptr, plan));
  if (!plan.sorted || plan.select_mode)
    return fail(CMI_GPU_ESTATE, "order_packets: a transport call of this "
                "engine %s", plan.sorted ? "orders a block's selection"
                                         : "does not order its packets");
  CMI_TRY(reserve_for(e, plan, n));
  ShootArgs a = shoot_args(e, plan, seed, iteration, first_packet, 0, n,
                           nullptr);
  CMI_TRY(order_packets(e, plan, a, n, nullptr));
  uint32_t *dkeys = nullptr;
  if (out_keys) {
    HIP_TRY(hipMalloc(&dkeys, sizeof(uint32_t) * n));
    const KeyArgs k = key_args(e, plan, a, n, nullptr);
    order_probe_kernel<<<grid_blocks(e, (int64_t)n, 8), CMI_BLOCK, 0,
                         e->stream>>>(k, a.order, dkeys);
  }
  hipError_t err = hipGetLastError();
  if (err == hipSuccess)
    err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess && out_ids)
    err = hipMemcpy(out_ids, a.order, sizeof(uint32_t) * n,
                    hipMemcpyDeviceToHost);
  if (err == hipSuccess && out_keys)
    err = hipMemcpy(out_keys, dkeys, sizeof(uint32_t) * n,
                    hipMemcpyDeviceToHost);
  (void)hipFree(dkeys);
  HIP_TRY(err);
  return CMI_GPU_OK;
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
    h.pad_sigma = e->model.xsec_fixed[ION_H_n];
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

/* LevelFrequencyBins::LevelFrequencyBins, src/LevelFrequencyBins.hpp:52-66:
 * the ionization energies of src/ElementData.hpp:39-105 (Hz) in ascending
 * order, closed by four times hydrogen's */
static void level_frequency_edges(double edges[CMI_NION + 1]) {
  const double energies[CMI_NION] = {
      3.28810279e+15, 5.94523574e+15, 5.89588678e+15, 1.15792700e+16,
      3.51435505e+15, 7.15759434e+15, 1.14732262e+16, 3.29284691e+15,
      8.49136314e+15, 5.21432028e+15, 9.90492110e+15, 5.64310422e+15,
      8.41222200e+15, 1.14182796e+16};
  for (int i = 0; i < CMI_NION; ++i)
    edges[i] = energies[i];
  std::sort(edges, edges + CMI_NION);
  edges[CMI_NION] = 4. * energies[ION_H_n];
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
  level_frequency_edges(t.level_edges);
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

/* cube and Lyman-alpha mode do not outlive the cell velocities, which the
 * renderers' header replaces (scatter_driver.h) */
static void dust_cube_mark_stale(cmi_gpu_engine *e, const char *why);

/* the ray-traced renderers: line images and cubes, sky maps and cubes, the
 * radio continuum */
#include "render_driver.h"

/* the Monte Carlo scattered-light modes: dust images and cubes, the cell
 * source, the sky camera, several views, Lyman alpha */
#include "scatter_driver.h"

/* ------------------------------------------------------- escape maps -- */

int cmi_gpu_set_escape_tally(cmi_gpu_engine *e, int32_t nlon, int32_t nmu,
                             const double *frame, int32_t nfreq,
                             int32_t bins_type, double minimum_frequency,
                             double maximum_frequency) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (nlon < 0)
    return fail(CMI_GPU_EINVAL, "set_escape_tally: %d longitude pixels",
                (int)nlon);
  EscapeDev s = EscapeDev();
  if (nlon > 0) {
    if (nmu < 1 || nfreq < 1 || !frame)
      return fail(CMI_GPU_EINVAL, "set_escape_tally: %d x %d pixels, %d "
                  "frequency bins%s", (int)nlon, (int)nmu, (int)nfreq,
                  frame ? "" : ", no frame");
    if (3 * (int64_t)nfreq * (int64_t)nlon * (int64_t)nmu > (1ll << 24))
      return fail(CMI_GPU_EINVAL, "set_escape_tally: 3 x %d bins x %d x %d "
                  "pixels are more than 2^24 sums", (int)nfreq, (int)nlon,
                  (int)nmu);
    if (!sky_frame_is_orthonormal(frame))
      return fail(CMI_GPU_EINVAL, "set_escape_tally: the frame is not "
                  "orthonormal to 1e-9");
    if (bins_type == CMI_BINS_LEVEL) {
      if (nfreq != CMI_NION)
        return fail(CMI_GPU_EINVAL, "set_escape_tally: level bins are %d "
                    "bins, %d asked for", CMI_NION, (int)nfreq);
    } else if (bins_type == CMI_BINS_LINEAR) {
      if (!std::isfinite(minimum_frequency) ||
          !std::isfinite(maximum_frequency) ||
          !(maximum_frequency > minimum_frequency))
        return fail(CMI_GPU_EINVAL, "set_escape_tally: empty frequency range");
      s.bins_min = minimum_frequency;
      s.bins_max = maximum_frequency;
      s.inverse_frequency_width =
          nfreq / (maximum_frequency - minimum_frequency);
    } else {
      return fail(CMI_GPU_EINVAL, "Unknown FrequencyBins type: %d",
                  (int)bins_type);
    }
    s.nlon = nlon;
    s.nmu = nmu;
    s.nfreq = nfreq;
    s.bins_type = bins_type;
    for (int i = 0; i < 9; ++i)
      s.frame[i] = frame[i];
    level_frequency_edges(s.level_edges);
  }
  HIP_TRY(hipSetDevice(e->device));
  /* (kernels of an earlier call may still add to the old array) */
  HIP_TRY(hipStreamSynchronize(e->stream));
  CMI_TRY(publish_escape(e, false));
  (void)hipFree(e->escape.sky);
  e->escape = EscapeDev();
  if (nlon == 0)
    return CMI_GPU_OK;
  const size_t bytes = sizeof(double) * 3 * (size_t)nfreq * (size_t)nlon *
                       (size_t)nmu;
  if (hipMalloc(&s.sky, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CMI_GPU_ENOMEM, "set_escape_tally: no memory for %zu bytes",
                bytes);
  }
  HIP_TRY(hipMemsetAsync(s.sky, 0, bytes, e->stream));
  e->escape = s;
  return CMI_GPU_OK;
}

static size_t escape_tally_doubles(const cmi_gpu_engine *e) {
  return 3 * (size_t)e->escape.nfreq * (size_t)e->escape.nlon *
         (size_t)e->escape.nmu;
}

int cmi_gpu_reset_escape_tally(cmi_gpu_engine *e) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (!e->escape.sky)
    return fail(CMI_GPU_ESTATE, "reset_escape_tally: no escape tally set");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemsetAsync(e->escape.sky, 0,
                         sizeof(double) * escape_tally_doubles(e), e->stream));
  return CMI_GPU_OK;
}

int cmi_gpu_download_escape_tally(cmi_gpu_engine *e, double *sky) {
  if (!e || !sky)
    return fail(CMI_GPU_EINVAL, "download_escape_tally: bad argument");
  if (!e->escape.sky)
    return fail(CMI_GPU_ESTATE, "download_escape_tally: no escape tally set");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(sky, e->escape.sky,
                         sizeof(double) * escape_tally_doubles(e),
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CMI_GPU_OK;
}

int cmi_gpu_escape_pixels(const double *frame, int32_t nlon, int32_t nmu,
                          int64_t n, const double *directions, int32_t *pixels,
                          double *centres) {
  if (!frame || nlon < 1 || nmu < 1 || n < 0 ||
      (n > 0 && (!directions || !pixels)))
    return fail(CMI_GPU_EINVAL, "escape_pixels: bad argument");
  if (!sky_frame_is_orthonormal(frame))
    return fail(CMI_GPU_EINVAL, "escape_pixels: the frame is not orthonormal "
                "to 1e-9");
  for (int64_t k = 0; k < n; ++k)
    pixels[k] = cmi_escape_pixel(frame, nlon, nmu, directions + 3 * k);
  if (centres) {
    for (int32_t i = 0; i < nlon; ++i)
      for (int32_t j = 0; j < nmu; ++j) {
        const double mu = -1. + (2. * j + 1.) / nmu;
        const double l = -M_PI + 2. * M_PI * (i + 0.5) / nlon;
        const double st = std::sqrt(1. - mu * mu);
        const double c[3] = {st * std::cos(l), st * std::sin(l), mu};
        double *out = centres + 3 * ((size_t)i * nmu + j);
        for (int a = 0; a < 3; ++a)
          out[a] = c[0] * frame[a] + c[1] * frame[3 + a] + c[2] * frame[6 + a];
      }
  }
  return CMI_GPU_OK;
}

int cmi_gpu_cross_sections(cmi_gpu_engine *e, int64_t n,
                           const double *frequencies, double *sigma) {
  if (!e || n < 0 || (n > 0 && (!frequencies || !sigma)))
    return fail(CMI_GPU_EINVAL, "cross_sections: bad argument");
  if (!e->have_xsec)
    return fail(CMI_GPU_ESTATE, "cross_sections: set cross sections first");
  const ModelDev host_model = host_model_of(e);
  for (int64_t k = 0; k < n; ++k)
    cmi_cross_sections(host_model, frequencies[k], sigma + CMI_NION * k);
  return CMI_GPU_OK;
}

} // extern "C"

/* ------------------------------------------------------ SPH mappings -- */

namespace {

/* device memory of one call */
struct SphScratch {
  std::vector<void *> blocks;
  ~SphScratch() {
    for (void *b : blocks)
      (void)hipFree(b);
  }
  template <typename T> int get(T **ptr, size_t count, const char *what) {
    void *b = nullptr;
    if (hipMalloc(&b, sizeof(T) * (count ? count : 1)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CMI_GPU_ENOMEM, "sph_map: no memory for %zu bytes of %s",
                  sizeof(T) * count, what);
    }
    blocks.push_back(b);
    *ptr = static_cast<T *>(b);
    return CMI_GPU_OK;
  }
};

/* device time between pairs of events, summed into the stats */
struct SphTimer {
  hipEvent_t events[4] = {nullptr, nullptr, nullptr, nullptr};
  int used = 0;
  ~SphTimer() {
    for (hipEvent_t ev : events)
      if (ev)
        (void)hipEventDestroy(ev);
  }
  void mark(hipStream_t stream) {
    if (used < 4 && hipEventCreate(&events[used]) == hipSuccess) {
      (void)hipEventRecord(events[used], stream);
      ++used;
    }
  }
  /* after the stream was synchronized */
  int64_t nanoseconds() const {
    double ms = 0.;
    for (int k = 0; k + 1 < used; k += 2) {
      float part = 0.f;
      if (hipEventElapsedTime(&part, events[k], events[k + 1]) == hipSuccess)
        ms += part;
    }
    return (int64_t)(ms * 1.e6);
  }
};

const char *const sph_decline_names[4] = {
    "taken", "no particles",
    "twice the largest reach is not below the smallest side of the periodic "
    "box",
    "the tile lists exceed the cap"};

int sph_declined(cmi_gpu_engine *e, const char *call, int reason) {
  e->sph_map_stats[6] = reason;
  return fail(CMI_GPU_EDECLINED, "%s declined: %s", call,
              sph_decline_names[reason]);
}

/* the arguments both mappings share; fills the geometry, uploads the
 * particles and returns the largest reach */
int sph_map_begin(cmi_gpu_engine *e, const char *call, int32_t form, int64_t n,
                  const double *positions, const double *h,
                  const double *periodic_box, const double *grid_anchor,
                  const double *grid_sides, const int32_t *ncell,
                  SphMapGeometry *g, SphScratch &mem, double **d_positions,
                  double **d_h) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  for (int k = 0; k < 8; ++k)
    e->sph_map_stats[k] = 0;
  e->sph_map_stats[3] = CMI_SPH_STAGE_CHUNK;
  if (form != CMI_SPH_FORM_SPLINE_H && form != CMI_SPH_FORM_SPLINE_2H)
    return fail(CMI_GPU_EINVAL, "%s: unknown kernel form %d", call, (int)form);
  if (n < 0 || !grid_anchor || !grid_sides || !ncell ||
      (n > 0 && (!positions || !h)))
    return fail(CMI_GPU_EINVAL, "%s: bad argument", call);
  for (int a = 0; a < 3; ++a) {
    if (ncell[a] < 1 || !(grid_sides[a] > 0.) || !std::isfinite(grid_sides[a]) ||
        !std::isfinite(grid_anchor[a]))
      return fail(CMI_GPU_EINVAL, "%s: bad grid", call);
    if (periodic_box &&
        (!(periodic_box[3 + a] > 0.) || !std::isfinite(periodic_box[3 + a])))
      return fail(CMI_GPU_EINVAL, "%s: bad periodic box", call);
  }
  if ((int64_t)ncell[0] * ncell[1] * ncell[2] >= ((int64_t)1 << 31) ||
      n >= ((int64_t)1 << 31))
    return fail(CMI_GPU_EINVAL, "%s: 2^31 cells or particles or more", call);
  double largest = 0.;
  for (int64_t i = 0; i < n; ++i) {
    if (!(h[i] > 0.) || !std::isfinite(h[i]) ||
        !std::isfinite(positions[3 * i]) ||
        !std::isfinite(positions[3 * i + 1]) ||
        !std::isfinite(positions[3 * i + 2]))
      return fail(CMI_GPU_EINVAL, "%s: particle %lld is not finite or has no "
                  "smoothing length", call, (long long)i);
    largest = std::max(largest, cmi_sph_reach(form, h[i]));
  }
  const int early =
      cmi_sph_decline_early(n, largest, periodic_box ? periodic_box + 3 : nullptr);
  if (early)
    return sph_declined(e, call, early);
  *g = cmi_sph_geometry(grid_anchor, grid_sides, ncell,
                        periodic_box ? periodic_box + 3 : nullptr);
  HIP_TRY(hipSetDevice(e->device));
  CMI_TRY(mem.get(d_positions, 3 * (size_t)n, "positions"));
  CMI_TRY(mem.get(d_h, (size_t)n, "smoothing lengths"));
  HIP_TRY(hipMemcpyAsync(*d_positions, positions, sizeof(double) * 3 * n,
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(*d_h, h, sizeof(double) * n, hipMemcpyHostToDevice,
                         e->stream));
  return CMI_GPU_OK;
}

template <int FORM, bool PERIODIC>
void sph_launch_cells(int K, int ntiles, hipStream_t stream,
                      const SphMapGeometry &g, int64_t n, const double *pos,
                      const double *h, const double *amp,
                      const unsigned int *offsets, const uint32_t *list,
                      double *out) {
  const dim3 grid(ntiles), block(CMI_SPH_TILE_CELLS);
  switch (K) {
  case 1:
    hipLaunchKernelGGL((sph_cells_kernel<FORM, 1, PERIODIC>), grid, block, 0,
                       stream, g, n, pos, h, amp, offsets, list, out);
    break;
  case 2:
    hipLaunchKernelGGL((sph_cells_kernel<FORM, 2, PERIODIC>), grid, block, 0,
                       stream, g, n, pos, h, amp, offsets, list, out);
    break;
  case 3:
    hipLaunchKernelGGL((sph_cells_kernel<FORM, 3, PERIODIC>), grid, block, 0,
                       stream, g, n, pos, h, amp, offsets, list, out);
    break;
  default:
    hipLaunchKernelGGL((sph_cells_kernel<FORM, 4, PERIODIC>), grid, block, 0,
                       stream, g, n, pos, h, amp, offsets, list, out);
    break;
  }
}

template <int FORM, bool PERIODIC>
void sph_launch_particles(hipStream_t stream, const SphMapGeometry &g,
                          int64_t nlane, const uint32_t *lane_ids,
                          int64_t nwave, const uint32_t *wave_ids,
                          const double *pos, const double *h,
                          const double *values, double *out) {
  if (nlane > 0)
    hipLaunchKernelGGL((sph_particles_lane_kernel<FORM, PERIODIC>),
                       dim3((unsigned)((nlane + 255) / 256)), dim3(256), 0,
                       stream, g, nlane, lane_ids, pos, h, values, out);
  if (nwave > 0)
    hipLaunchKernelGGL((sph_particles_wave_kernel<FORM, PERIODIC>),
                       dim3((unsigned)((nwave + 3) / 4)), dim3(256), 0, stream,
                       g, nwave, wave_ids, pos, h, values, out);
}

} // namespace

extern "C" {

int cmi_gpu_sph_map_to_cells(cmi_gpu_engine *e, int32_t form, int64_t n,
                             const double *positions, const double *h,
                             int32_t K, const double *amplitudes,
                             const double *periodic_box,
                             const double *grid_anchor,
                             const double *grid_sides, const int32_t *ncell,
                             double *out) {
  static const char call[] = "sph_map_to_cells";
  if (K < 1 || K > CMI_SPH_MAX_AMPLITUDES || !out || (n > 0 && !amplitudes))
    return fail(CMI_GPU_EINVAL, "%s: bad argument (%d amplitude arrays)", call,
                (int)K);
  SphMapGeometry g;
  SphScratch mem;
  double *d_pos = nullptr, *d_h = nullptr;
  CMI_TRY(sph_map_begin(e, call, form, n, positions, h, periodic_box,
                        grid_anchor, grid_sides, ncell, &g, mem, &d_pos, &d_h));
  const size_t ncells = (size_t)ncell[0] * ncell[1] * ncell[2];
  const size_t ntiles = (size_t)g.ntile[0] * g.ntile[1] * g.ntile[2];
  e->sph_map_stats[0] = (int64_t)ntiles;

  /* count, scan (host), fill */
  unsigned int *d_counts = nullptr, *d_offsets = nullptr;
  CMI_TRY(mem.get(&d_counts, ntiles, "tile counts"));
  CMI_TRY(mem.get(&d_offsets, ntiles + 1, "tile offsets"));
  HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(unsigned int) * ntiles, e->stream));
  const dim3 pgrid((unsigned)((n + 255) / 256)), pblock(256);
  SphTimer timer;
  timer.mark(e->stream);
  if (form == CMI_SPH_FORM_SPLINE_H)
    hipLaunchKernelGGL((sph_tile_count_kernel<0>), pgrid, pblock, 0, e->stream,
                       g, n, d_pos, d_h, d_counts);
  else
    hipLaunchKernelGGL((sph_tile_count_kernel<1>), pgrid, pblock, 0, e->stream,
                       g, n, d_pos, d_h, d_counts);
  HIP_TRY(hipGetLastError());
  timer.mark(e->stream);
  std::vector<unsigned int> counts(ntiles), offsets(ntiles + 1);
  HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, sizeof(unsigned int) * ntiles,
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int64_t entries = 0, longest = 0;
  for (size_t t = 0; t < ntiles; ++t) {
    entries += counts[t];
    longest = std::max<int64_t>(longest, counts[t]);
  }
  e->sph_map_stats[1] = entries;
  e->sph_map_stats[2] = longest;
  if (cmi_sph_decline_lists(entries, CMI_SPH_LIST_CAP))
    return sph_declined(e, call, CMI_SPH_DECLINE_LIST_SIZE);
  offsets[0] = 0;
  for (size_t t = 0; t < ntiles; ++t)
    offsets[t + 1] = offsets[t] + counts[t];

  uint32_t *d_list = nullptr;
  double *d_amp = nullptr, *d_out = nullptr;
  CMI_TRY(mem.get(&d_list, (size_t)entries, "tile lists"));
  CMI_TRY(mem.get(&d_amp, (size_t)K * n, "amplitudes"));
  CMI_TRY(mem.get(&d_out, (size_t)K * ncells, "cell sums"));
  HIP_TRY(hipMemsetAsync(d_list, 0, sizeof(uint32_t) * (entries ? entries : 1),
                         e->stream));
  HIP_TRY(hipMemcpyAsync(d_offsets, offsets.data(),
                         sizeof(unsigned int) * (ntiles + 1),
                         hipMemcpyHostToDevice, e->stream));
  /* the cursors: the counts' array, set to the offsets */
  HIP_TRY(hipMemcpyAsync(d_counts, offsets.data(), sizeof(unsigned int) * ntiles,
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d_amp, amplitudes, sizeof(double) * (size_t)K * n,
                         hipMemcpyHostToDevice, e->stream));
  timer.mark(e->stream);
  if (form == CMI_SPH_FORM_SPLINE_H)
    hipLaunchKernelGGL((sph_tile_fill_kernel<0>), pgrid, pblock, 0, e->stream,
                       g, n, d_pos, d_h, d_counts, d_offsets + 1, d_list);
  else
    hipLaunchKernelGGL((sph_tile_fill_kernel<1>), pgrid, pblock, 0, e->stream,
                       g, n, d_pos, d_h, d_counts, d_offsets + 1, d_list);
  HIP_TRY(hipGetLastError());
  if (form == CMI_SPH_FORM_SPLINE_H) {
    if (g.periodic)
      sph_launch_cells<0, true>(K, (int)ntiles, e->stream, g, n, d_pos, d_h,
                                d_amp, d_offsets, d_list, d_out);
    else
      sph_launch_cells<0, false>(K, (int)ntiles, e->stream, g, n, d_pos, d_h,
                                 d_amp, d_offsets, d_list, d_out);
  } else {
    if (g.periodic)
      sph_launch_cells<1, true>(K, (int)ntiles, e->stream, g, n, d_pos, d_h,
                                d_amp, d_offsets, d_list, d_out);
    else
      sph_launch_cells<1, false>(K, (int)ntiles, e->stream, g, n, d_pos, d_h,
                                 d_amp, d_offsets, d_list, d_out);
  }
  HIP_TRY(hipGetLastError());
  timer.mark(e->stream);
  HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)K * ncells,
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->sph_map_stats[7] = timer.nanoseconds();
  return CMI_GPU_OK;
}

int cmi_gpu_sph_map_to_particles(cmi_gpu_engine *e, int32_t form, int64_t n,
                                 const double *positions, const double *h,
                                 const double *periodic_box,
                                 const double *grid_anchor,
                                 const double *grid_sides,
                                 const int32_t *ncell,
                                 const double *cell_values, double *out) {
  static const char call[] = "sph_map_to_particles";
  if (!cell_values || (n > 0 && !out))
    return fail(CMI_GPU_EINVAL, "%s: bad argument", call);
  SphMapGeometry g;
  SphScratch mem;
  double *d_pos = nullptr, *d_h = nullptr;
  CMI_TRY(sph_map_begin(e, call, form, n, positions, h, periodic_box,
                        grid_anchor, grid_sides, ncell, &g, mem, &d_pos, &d_h));
  const size_t ncells = (size_t)ncell[0] * ncell[1] * ncell[2];

  /* the class split */
  std::vector<uint32_t> ids((size_t)n);
  int64_t nlane = 0, nwave = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t candidates = cmi_sph_particle_candidates(
        g, positions + 3 * i, cmi_sph_reach(form, h[i]));
    const int cls = cmi_sph_particle_class(candidates);
    if (cls == 1)
      ids[nlane++] = (uint32_t)i; /* from the front */
    else if (cls == 2)
      ids[n - 1 - nwave++] = (uint32_t)i; /* from the back */
  }
  e->sph_map_stats[4] = nwave;
  e->sph_map_stats[5] = nlane;

  uint32_t *d_ids = nullptr;
  double *d_values = nullptr, *d_out = nullptr;
  CMI_TRY(mem.get(&d_ids, (size_t)n, "class lists"));
  CMI_TRY(mem.get(&d_values, ncells, "cell values"));
  CMI_TRY(mem.get(&d_out, (size_t)n, "particle sums"));
  HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), sizeof(uint32_t) * n,
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d_values, cell_values, sizeof(double) * ncells,
                         hipMemcpyHostToDevice, e->stream));
  /* (a particle without a candidate midpoint is in neither class) */
  HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(double) * n, e->stream));
  const uint32_t *lane_ids = d_ids, *wave_ids = d_ids + (n - nwave);
  SphTimer timer;
  timer.mark(e->stream);
  if (form == CMI_SPH_FORM_SPLINE_H) {
    if (g.periodic)
      sph_launch_particles<0, true>(e->stream, g, nlane, lane_ids, nwave,
                                    wave_ids, d_pos, d_h, d_values, d_out);
    else
      sph_launch_particles<0, false>(e->stream, g, nlane, lane_ids, nwave,
                                     wave_ids, d_pos, d_h, d_values, d_out);
  } else {
    if (g.periodic)
      sph_launch_particles<1, true>(e->stream, g, nlane, lane_ids, nwave,
                                    wave_ids, d_pos, d_h, d_values, d_out);
    else
      sph_launch_particles<1, false>(e->stream, g, nlane, lane_ids, nwave,
                                     wave_ids, d_pos, d_h, d_values, d_out);
  }
  HIP_TRY(hipGetLastError());
  timer.mark(e->stream);
  HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->sph_map_stats[7] = timer.nanoseconds();
  return CMI_GPU_OK;
}

int cmi_gpu_get_sph_map_stats(cmi_gpu_engine *e, int64_t *stats) {
  if (!e || !stats)
    return fail(CMI_GPU_EINVAL, "get_sph_map_stats: bad argument");
  for (int k = 0; k < 8; ++k)
    stats[k] = e->sph_map_stats[k];
  return CMI_GPU_OK;
}

} // extern "C"

#include "group.h"
