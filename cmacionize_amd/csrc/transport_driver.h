/*
 * transport_driver.h - the host side of a transport call (included from
 * engine.hip): the buffers it needs, the launch plan of a call - which builds
 * of the kernels run, with what launch sizes and sort keys - and the stages of
 * one launch: a block's own packets, keys and sort, the first generation, the
 * tile rounds and the passes of the later generations.
 */
#ifndef CMI_TRANSPORT_DRIVER_H
#define CMI_TRANSPORT_DRIVER_H

/* make sure the sort buffers hold n packets, in a block of at least `words`
 * 32-bit words (what the bucket order of such a launch lays into it; the
 * radix sort needs 4 n) */
static int reserve_sort_buffers(cmi_gpu_engine *e, uint64_t n,
                                uint64_t words = 0) {
  if (e->sort_capacity >= n && e->sort_block_words >= words)
    return CMI_GPU_OK;
  if (n < e->sort_capacity)
    n = e->sort_capacity;
  if (words < 4 * n)
    words = 4 * n;
  HIP_TRY(hipStreamSynchronize(e->stream));
  (void)hipFree(e->sort_keys[0]);
  (void)hipFree(e->sort_temp);
  e->sort_keys[0] = nullptr;
  e->sort_temp = nullptr;
  e->sort_capacity = 0;
  e->sort_block_words = 0;
  uint32_t *block = nullptr;
  HIP_TRY(hipMalloc(&block, sizeof(uint32_t) * words));
  e->sort_block_words = words;
  e->sort_keys[0] = block;
  e->sort_keys[1] = block + n;
  e->sort_ids[0] = block + 2 * n;
  e->sort_ids[1] = block + 3 * n;
  size_t bytes = 0;
  HIP_TRY(cmi_sort_pairs_temp_bytes(n, 32, &bytes));
  e->sort_temp_bytes = bytes;
  HIP_TRY(hipMalloc(&e->sort_temp, bytes ? bytes : 16));
  e->sort_capacity = n;
  return CMI_GPU_OK;
}

/* make sure the two re-emission queues hold n packets each */
static int reserve_queues(cmi_gpu_engine *e, uint64_t n) {
  if (e->queue_capacity >= n)
    return CMI_GPU_OK;
  /* ended flights: pos[3], nu + cell, id, meta = 5.5 doubles per packet;
   * ready flights: pos[3], dir[3], tau, nu + id, meta = 9 doubles per packet;
   * every packet of a launch can be in either */
  const size_t ended_doubles = 6, ready_doubles = 9;
  CMI_TRY(grow(e, e->queue_block, e->queue_capacity, n,
               sizeof(double) * (ended_doubles + ready_doubles) * n));
  if (!e->queue_counts) {
    HIP_TRY(hipMalloc(&e->queue_counts, 2 * sizeof(unsigned int)));
  }
  QueueDev &q = e->ended_queue;
  double *base = e->queue_block;
  for (int a = 0; a < 3; ++a) {
    q.pos[a] = base + (size_t)a * n;
    q.dir[a] = nullptr;
  }
  q.tau = nullptr;
  q.nu = base + (size_t)3 * n;
  q.cell = (int32_t *)(base + (size_t)4 * n);
  q.id = (uint32_t *)q.cell + n;
  q.meta = q.id + n;
  q.count = e->queue_counts;
  QueueDev &r = e->ready_queue;
  base = e->queue_block + ended_doubles * n;
  for (int a = 0; a < 3; ++a) {
    r.pos[a] = base + (size_t)a * n;
    r.dir[a] = base + (size_t)(3 + a) * n;
  }
  r.tau = base + (size_t)6 * n;
  r.nu = base + (size_t)7 * n;
  r.cell = nullptr;
  r.id = (uint32_t *)(base + (size_t)8 * n);
  r.meta = r.id + n;
  r.count = e->queue_counts + 1;
  return CMI_GPU_OK;
}

/* tiles of the engine's grid for the current transport flavour */
static TileGridDev tile_grid(const cmi_gpu_engine *e) {
  TileGridDev t;
  const bool heat = e->config.track_heating != 0;
  if (e->full_ions) {
    t.log2[0] = TileShape<true, true>::LX;
    t.log2[1] = TileShape<true, true>::LY;
    t.log2[2] = TileShape<true, true>::LZ;
  } else if (heat) {
    t.log2[0] = TileShape<false, true>::LX;
    t.log2[1] = TileShape<false, true>::LY;
    t.log2[2] = TileShape<false, true>::LZ;
  } else {
    t.log2[0] = TileShape<false, false>::LX;
    t.log2[1] = TileShape<false, false>::LY;
    t.log2[2] = TileShape<false, false>::LZ;
  }
  int64_t total = 1;
  for (int a = 0; a < 3; ++a) {
    const int side = 1 << t.log2[a];
    t.ntile[a] = (e->grid.ncell[a] + side - 1) / side;
    total *= t.ntile[a];
  }
  t.ntiles = (int32_t)total;
  return t;
}

/* make sure the flight rows of the tile rounds hold n flights each */
static int reserve_tile_buffers(cmi_gpu_engine *e, uint64_t n) {
  const bool weights = e->full_ions;
  if (e->tile_capacity >= n && (e->tile_has_weights || !weights))
    return CMI_GPU_OK;
  HIP_TRY(hipStreamSynchronize(e->stream));
  (void)hipFree(e->tile_block);
  e->tile_block = nullptr;
  e->tile_capacity = 0;
  const TileGridDev t = tile_grid(e);
  const size_t row_bytes = sizeof(double) * CMI_FLIGHT_DOUBLES * n;
  const size_t weight_bytes = weights ? sizeof(double) * CMI_NACC * n : 0;
  const size_t key_bytes = (sizeof(uint32_t) * n + 255) & ~(size_t)255;
  const size_t nitems =
      (size_t)t.ntiles + n / CMI_TILE_ITEM_FLIGHTS_FULL + 4;
  const size_t item_bytes = sizeof(TileItemDev) * nitems;
  const size_t begin_bytes =
      (sizeof(uint32_t) * ((size_t)t.ntiles + 2) + 255) & ~(size_t)255;
  const size_t count_bytes =
      (sizeof(unsigned int) * nitems + 255) & ~(size_t)255;
  const bool counting = t.ntiles <= CMI_TILE_SORT_MAX_TILES;
  const size_t hist_bytes =
      counting ? sizeof(uint32_t) * (size_t)t.ntiles * CMI_TILE_SORT_BLOCKS : 0;
  const size_t total = 2 * (row_bytes + weight_bytes + key_bytes) +
                       6 * key_bytes + 2 * begin_bytes + 2 * count_bytes +
                       item_bytes + hist_bytes;
  HIP_TRY(hipMalloc(&e->tile_block, total));
  if (!e->tile_counts)
    HIP_TRY(hipMalloc(&e->tile_counts, 8 * sizeof(unsigned int)));
  char *at = e->tile_block;
  for (int k = 0; k < 2; ++k) {
    FlightRowsDev &r = e->tile_rows[k];
    r.rows = (double *)at;
    at += row_bytes;
    r.weights = weights ? (double *)at : nullptr;
    at += weight_bytes;
    r.keys = (uint32_t *)at;
    at += key_bytes;
    r.count = e->tile_counts + k;
    r.capacity = (unsigned int)n;
  }
  e->tile_iota = (uint32_t *)at;
  at += key_bytes;
  e->tile_ended_slot = (uint32_t *)at;
  at += key_bytes;
  e->tile_ended_pos = (uint32_t *)at;
  at += key_bytes;
  for (int k = 0; k < 2; ++k) {
    e->tile_slot_of[k] = (uint32_t *)at;
    at += key_bytes;
  }
  e->tile_new_slots = (uint32_t *)at;
  at += key_bytes;
  e->tile_begin = (uint32_t *)at;
  at += begin_bytes;
  e->tile_total = counting ? (uint32_t *)at : nullptr;
  at += begin_bytes;
  e->tile_absorbed_count = (unsigned int *)at;
  at += count_bytes;
  e->tile_absorbed_before = (unsigned int *)at;
  at += count_bytes;
  e->tile_items = (TileItemDev *)at;
  at += item_bytes;
  e->tile_blockhist = counting ? (uint32_t *)at : nullptr;
  iota_kernel<<<grid_blocks(e, (int64_t)n, 8), CMI_BLOCK, 0, e->stream>>>(
      e->tile_iota, n);
  HIP_TRY(hipGetLastError());
  e->tile_capacity = n;
  e->tile_has_weights = weights;
  return CMI_GPU_OK;
}

/* A block of a decomposed grid flies the packets that start in it (after at
 * most one step of length zero, see shoot_kernel): no source within one cell
 * of the block - and, for the block at the grid's origin, none outside the
 * whole grid - means nothing to emit, and the pass over the packet ids can be
 * skipped altogether. */
static bool block_emits_nothing(const cmi_gpu_engine *e) {
  if (e->model.continuous_type != 0)
    return false; /* its packets enter through every face of the box */
  const GridDev &g = e->grid;
  const bool at_origin = (g.offset[0] | g.offset[1] | g.offset[2]) == 0;
  for (int32_t s = 0; s < e->model.nsource; ++s) {
    bool near = true, in_grid = true;
    for (int a = 0; a < 3; ++a) {
      const double x = e->source_position_host[3 * (size_t)s + a];
      const double lo = g.anchor[a] + g.cellside[a] * (g.offset[a] - 1);
      const double hi =
          g.anchor[a] + g.cellside[a] * (g.offset[a] + g.ncell[a] + 1);
      near &= (x >= lo && x <= hi);
      /* (a cell of margin: the kernel decides by cell index) */
      in_grid &= (x >= g.anchor[a] + g.cellside[a] &&
                  x <= g.anchor[a] + g.box_sides[a] - g.cellside[a]);
    }
    if (near || (!in_grid && at_origin))
      return false;
  }
  return e->model.nsource > 0;
}

static uint64_t reemit_inline_below(const cmi_gpu_engine *e) {
  if (e->tune.reemit_inline_below >= 0)
    return (uint64_t)e->tune.reemit_inline_below;
  return e->grid.decomposed ? 262144u : 4096u;
}

typedef void (*ShootKernel)(const ShootArgs);
typedef void (*TileKernel)(const TileArgs);
typedef void (*PointKernel)(const ShootArgs, const PointEmitDev *);

/* the build of shoot_kernel that flies the first generation of new packets:
 * the one of the later generations, or one of the specialised builds */
enum FirstBuild {
  FIRST_GENERIC,
  /* a non-periodic grid with the block combining table (every benchmark
   * config) */
  FIRST_TABLE,
  /* ... and, hydrogen only, marching through padded records */
  FIRST_PAD,
  /* ... in the larger blocks for grids of more than CMI_TABLE_BIG_CELLS cells
   * (pad_big) */
  FIRST_PAD_BIG,
  /* ... or, for multi-ion runs whose packets are sorted anyway, with the
   * emission physics done by the key kernel (the rows live in the second
   * weights buffer of the tile rounds, idle during the first generation) */
  FIRST_PRE
};

/* Everything a transport call decides before its first launch. */
struct LaunchPlan {
  bool heat, reemit;
  bool exact;       /* the exact marcher, not the incremental one */
  bool tracking;    /* spectrum trackers count */
  bool passes;      /* re-emission in passes, not in place */
  bool tiles;       /* later generations in tile rounds */
  bool sorted;      /* new packets, ordered by direction */
  bool select_mode; /* a block picks its own packets out of each launch's ids */
  int agg, agg_reemit;
  FirstBuild first;
  bool pad, pad_big;     /* first is FIRST_PAD or FIRST_PAD_BIG / the latter */
  /* pad, no heating term, and every packet of the call carries one weight:
   * the UNIFORM build, whose table sums path lengths; weight x sigma_H */
  bool pad_uniform;
  double uniform_scale;
  int64_t padded_cells;
  /* pad, and every refill of the launch fills a whole idle wave from one
   * claimed chunk of 64 new packets that fly to their end where they are: the
   * bundle build (shoot_bundle_kernel) */
  bool bundle;
  /* bundle and pad_uniform, and every packet comes from one discrete source
   * (PacketOrigin::fixed): the point build of the bundle kernel */
  bool bundle_point;
  PointKernel kernel_point; /* (in place of kernel_first) */
  /* the kernel of a pass, the one that follows re-emissions in place, and the
   * first generation's, with their workgroups per CU */
  ShootKernel kernel, kernel_inline, kernel_first;
  int blocks_per_cu, blocks_per_cu_inline, blocks_per_cu_first;
  int first_threads;
  /* sort key: direction bits, the tau class and the source index */
  uint32_t tau_bits, source_bits, dir_bits;
  int key_bits;
  double sigma_ref;
  /* the launches that are large enough get their order from the bucket
   * order (packet_order.h; bucket_plan_of decides per launch), the others
   * and every launch of the other plans from key kernel and radix sort */
  bool bucket_order;
  TileKernel tile_kernel;
  int tile_threads, tile_blocks_per_cu;
};

/* The build of shoot_kernel for a set of flags. `first` other than
 * FIRST_GENERIC names a first-generation build (PAD: hydrogen only, PRE:
 * multi-ion only); `track` is the incremental marcher with the trackers' hook.
 * These tables are all the builds there are, listed in the order the code
 * object holds them. */
static ShootKernel shoot_build(bool full, bool heat, bool reemit, bool exact,
                               bool track, FirstBuild first,
                               bool uniform = false) {
  /* [exact][2 full + heat][reemit] */
  static const ShootKernel generic[2][4][2] = {
      {{shoot_kernel<false, false, false, false>,
        shoot_kernel<false, false, true, false>},
       {shoot_kernel<false, true, false, false>,
        shoot_kernel<false, true, true, false>},
       {shoot_kernel<true, false, false, false>,
        shoot_kernel<true, false, true, false>},
       {shoot_kernel<true, true, false, false>,
        shoot_kernel<true, true, true, false>}},
      {{shoot_kernel<false, false, false, true>,
        shoot_kernel<false, false, true, true>},
       {shoot_kernel<false, true, false, true>,
        shoot_kernel<false, true, true, true>},
       {shoot_kernel<true, false, false, true>,
        shoot_kernel<true, false, true, true>},
       {shoot_kernel<true, true, false, true>,
        shoot_kernel<true, true, true, true>}}};
  /* [2 full + heat][reemit] */
  static const ShootKernel tracked[4][2] = {
      {shoot_kernel<false, false, false, false, false, false, false, true>,
       shoot_kernel<false, false, true, false, false, false, false, true>},
      {shoot_kernel<false, true, false, false, false, false, false, true>,
       shoot_kernel<false, true, true, false, false, false, false, true>},
      {shoot_kernel<true, false, false, false, false, false, false, true>,
       shoot_kernel<true, false, true, false, false, false, false, true>},
      {shoot_kernel<true, true, false, false, false, false, false, true>,
       shoot_kernel<true, true, true, false, false, false, false, true>}};
  /* [!full][!heat] */
  static const ShootKernel table[2][2] = {
      {shoot_kernel<true, true, false, false, true>,
       shoot_kernel<true, false, false, false, true>},
      {shoot_kernel<false, true, false, false, true>,
       shoot_kernel<false, false, false, false, true>}};
  /* [!heat + uniform] (UNIFORM: the eighth flag of a PAD kernel) */
  static const ShootKernel pad_big[3] = {
      shoot_kernel<false, true, false, false, true, false, true, false, true>,
      shoot_kernel<false, false, false, false, true, false, true, false, true>,
      shoot_kernel<false, false, false, false, true, false, true, true, true>};
  static const ShootKernel pad[3] = {
      shoot_kernel<false, true, false, false, true, false, true>,
      shoot_kernel<false, false, false, false, true, false, true>,
      shoot_kernel<false, false, false, false, true, false, true, true>};
  static const ShootKernel pre[2] = {
      shoot_kernel<true, true, false, false, true, true>,
      shoot_kernel<true, false, false, false, true, true>};
  switch (first) {
  case FIRST_TABLE:
    return table[!full][!heat];
  case FIRST_PAD:
    return pad[!heat + (!heat && uniform)];
  case FIRST_PAD_BIG:
    return pad_big[!heat + (!heat && uniform)];
  case FIRST_PRE:
    return pre[!heat];
  case FIRST_GENERIC:
    break;
  }
  return track ? tracked[2 * full + heat][reemit]
               : generic[exact][2 * full + heat][reemit];
}

/* (a template: engine.hip includes this file inside its extern "C") */
extern "C++" {
/* workgroups of `kernel` a CU holds: at least one, at most `most` */
template <class Kernel>
static int blocks_per_cu_of(Kernel kernel, int threads, int most, int &out) {
  out = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out, kernel, threads,
                                                       0));
  if (out < 1)
    out = 1;
  if (out > most)
    out = most;
  return CMI_GPU_OK;
}
} // extern "C++"

/* The plan of a call that transports n_packets new packets (flights == NULL)
 * or handed-over flights. */
static int plan_launches(cmi_gpu_engine *e, uint64_t n_packets,
                         const double *flights, LaunchPlan &p) {
  const cmi_gpu_engine::Tuning &tune = e->tune;
  p.heat = e->config.track_heating != 0;
  p.reemit = e->model.reemit_type != CMI_GPU_REEMIT_NONE;
  /* cross-lane aggregation keys and the fast marcher use 32-bit cell
   * indices, and the marcher a 32-bit BYTE offset into the 16-B transport
   * records (fast_load_record): 2^28 cells. Larger engines (768^3 and up;
   * 2^28 cells are 73 GB of state) march with the exact marcher. */
  const bool small_grid = e->ncell < CMI_FAST_MARCHER_MAX_CELLS;
  p.agg = small_grid ? tune.aggregate : CMI_AGG_NONE;
  p.agg_reemit = small_grid ? tune.aggregate_reemit : CMI_AGG_NONE;
  /* (a set escape tally counts like a set tracker) */
  p.tracking = e->trackers_enabled &&
               (e->trackers.n != 0 || e->escape.sky != nullptr);
  /* (trackers count in the exact marcher on an undivided grid - the counts
   * equal the oracle's one by one - and in the incremental one on the blocks
   * of a decomposed grid, whose hand-overs carry its state) */
  p.exact = tune.exact_dda || !small_grid ||
            (p.tracking && !e->grid.decomposed);
  /* with re-emission in passes the transport launches use the variant WITHOUT
   * the re-emission code (absorbed packets go to the interaction kernel); the
   * variant with it follows re-emissions in place */
  /* (a handful of handed-over flights - the late hand-over rounds of a
   * decomposed grid - are followed in place, re-emissions and all, by ONE
   * launch: a pass, the interaction kernel and the in-place kernel after it
   * each cost the latency of the longest flight, ~1 ms, whatever their
   * number) */
  p.passes = p.reemit && tune.reemit_passes &&
             !(flights && n_packets < reemit_inline_below(e));
  p.sorted = tune.sort_packets && !flights;
  /* later generations in tile rounds: needs the incremental marcher */
  p.tiles = p.passes && tune.tile_rounds && !p.exact && !p.tracking;
  /* a block of a decomposed grid picks its own packets out of each launch's
   * ids first (block_select_kernel): buffers for what it picks, not for all
   * ids (1 / 8 of them in config 5 - sort buffers, queues and flight slots
   * are 40 GB per 1e8 packets) */
  p.select_mode = p.sorted && e->grid.decomposed;

  /* the first generation of new packets on a non-periodic grid with the
   * block combining table (every benchmark config): the specialised build of
   * the same kernel */
  const bool table =
      !flights && !p.exact && !p.tracking && p.agg == CMI_AGG_BLOCK &&
      (p.passes || !p.reemit) &&
      !(e->grid.periodic[0] | e->grid.periodic[1] | e->grid.periodic[2]);
  /* (the kernel addresses padded records by 32-bit byte offsets:
   * (nx + 2)(ny + 2)(nz + 2) < 2^29, which a flat grid of fewer than 2^28
   * cells - 1 x 13400 x 13400 - can exceed) */
  p.padded_cells = ((int64_t)e->grid.ncell[0] + 2 * CMI_PAD_LAYERS) *
                   ((int64_t)e->grid.ncell[1] + 2 * CMI_PAD_LAYERS) *
                   ((int64_t)e->grid.ncell[2] + 2 * CMI_PAD_LAYERS);
  /* (a block of a decomposed grid: its ghost layer says "left the block", the
   * end of the flight then decides between "left the box" and a hand-over) */
  /* The padded records hold sigma_H n x_H (cmi_pad_record): the cross section
   * must be one number for the call, not negative (a record's sign bit says
   * "no gas") and finite. !full_ions is that guarantee (update_full_flag): the
   * cross sections are the fixed ones and only hydrogen's is non-zero, so
   * set_cross_sections gives every packet xsec_fixed[ION_H_n], whatever its
   * frequency or source; handed-over flights and re-emitted packets never
   * come here (table: !flights, passes or no re-emission). */
  const double sigma_H = e->model.xsec_fixed[ION_H_n];
  p.pad = table && !e->full_ions && tune.pad_march &&
          p.padded_cells < ((int64_t)1 << 29) && sigma_H >= 0. &&
          std::isfinite(sigma_H);
  p.pad_big = p.pad && e->ncell > CMI_TABLE_BIG_CELLS;
  /* one weight for every packet of the call: all from the discrete sources
   * (photon_weight[0]), all from the continuous one ([1]: emit_geometry
   * draws the origin against continuous_probability), or both weights equal.
   * The kernels with the heating term keep the product per lane. */
  const double pc = e->model.continuous_probability;
  const double *pw = e->model.photon_weight;
  p.pad_uniform = p.pad && !p.heat && tune.pad_uniform &&
                  (pc <= 0. || pc >= 1. || pw[0] == pw[1]);
  /* (the product the per-lane build forms: weight x sigma_H) */
  p.uniform_scale = (pc >= 1. ? pw[1] : pw[0]) * sigma_H;
  p.first = FIRST_GENERIC;
  if (p.pad)
    p.first = p.pad_big ? FIRST_PAD_BIG : FIRST_PAD;
  else if (table && e->full_ions && tune.pre_emission && p.sorted &&
           p.tiles)
    p.first = FIRST_PRE;
  else if (table)
    p.first = FIRST_TABLE;
  /* (the hydrogen-only kernels built for the table run in larger blocks) */
  p.first_threads = (table && !e->full_ions)
                        ? (p.pad_big ? shoot_block_threads<false, true, true>()
                                     : shoot_block_threads<false, true>())
                        : CMI_BLOCK;

  const bool track = p.tracking && !p.exact;
  /* (a block of a decomposed grid: the hook in the incremental marcher) */
  p.kernel_inline =
      shoot_build(e->full_ions, p.heat, true, p.exact, track, FIRST_GENERIC);
  p.kernel = (p.reemit && !p.passes)
                 ? p.kernel_inline
                 : shoot_build(e->full_ions, p.heat, false, p.exact, track,
                               FIRST_GENERIC);
  p.kernel_first = table ? shoot_build(e->full_ions, p.heat, false, false,
                                       false, p.first, p.pad_uniform)
                         : p.kernel;
  /* The bundle build of the padded march (tuning "bundle_march"): new packets
   * from ids (table: !flights), claimed spans of chunks of 64 that a wave
   * takes only when all its lanes are idle, an undivided grid in the smaller
   * blocks, no heating term, and no re-emission - in passes it would park the
   * absorbed packets, in place the table is not taken at all. Everything else
   * keeps the general kernels. */
  p.bundle = p.pad && !p.pad_big && !p.heat && !p.reemit &&
             !e->grid.decomposed && tune.span_claim && tune.chunk == 64 &&
             tune.refill_threshold == 64 && tune.bundle_march;
  if (p.bundle)
    p.kernel_first = p.pad_uniform ? shoot_bundle_kernel<true>
                                   : shoot_bundle_kernel<false>;
  /* ... and its point build (tuning "bundle_point"): PacketOrigin::fixed, as
   * the host knows it - no continuous source, one discrete one (whose
   * cumulative weight cmi_gpu_set_sources sets to 1) */
  p.bundle_point = p.bundle && p.pad_uniform && tune.bundle_point &&
                   e->model.continuous_probability == 0. &&
                   e->model.nsource == 1;
  p.kernel_point = p.bundle_point ? shoot_bundle_kernel<true, true> : nullptr;
  CMI_TRY(blocks_per_cu_of(p.kernel, CMI_BLOCK, tune.max_blocks_per_cu,
                           p.blocks_per_cu));
  CMI_TRY(blocks_per_cu_of(p.kernel_inline, CMI_BLOCK, tune.max_blocks_per_cu,
                           p.blocks_per_cu_inline));
  /* (the specialised first-generation kernels may fit more blocks per CU) */
  p.blocks_per_cu_first = p.blocks_per_cu;
  if (p.bundle_point)
    CMI_TRY(blocks_per_cu_of(p.kernel_point, p.first_threads,
                             tune.max_blocks_per_cu, p.blocks_per_cu_first));
  else if (table)
    CMI_TRY(blocks_per_cu_of(p.kernel_first, p.first_threads,
                             tune.max_blocks_per_cu, p.blocks_per_cu_first));
  p.tile_kernel = nullptr;
  p.tile_threads = p.tile_blocks_per_cu = 0;
  if (p.tiles) {
    if (e->full_ions)
      p.tile_kernel =
          p.heat ? tile_kernel<true, true> : tile_kernel<true, false>;
    else
      p.tile_kernel =
          p.heat ? tile_kernel<false, true> : tile_kernel<false, false>;
    p.tile_threads = e->full_ions
                         ? TileShape<true, true>::THREADS
                         : (p.heat ? TileShape<false, true>::THREADS
                                   : TileShape<false, false>::THREADS);
    CMI_TRY(blocks_per_cu_of(p.tile_kernel, p.tile_threads, INT_MAX,
                             p.tile_blocks_per_cu));
  }

  /* sort key: 22 direction bits, the tau class and the source index. The
   * tau classes only help when a packet's range follows from its optical
   * depth alone (one cross section for all packets). */
  const uint64_t max_launch = tune.max_packets_per_launch;
  const uint64_t per_source =
      (n_packets < max_launch ? n_packets : max_launch) /
      (uint64_t)(e->model.nsource > 0 ? e->model.nsource : 1);
  if (tune.sort_tau_bits >= 0)
    p.tau_bits = (uint32_t)tune.sort_tau_bits;
  else
    /* measured on 256^3: the classes pay off once a direction bin of
     * 64 x 2^bits packets is still narrower than a few cells */
    /* (multi-ion runs since round 5's cell-by-cell sums: 0 / 1 / 2 / 3 /
     * 4 class bits 71.8 / 70.0 / 66.3 / 68.0 / 68.0 ms per 1e8 packets) */
    p.tau_bits = per_source >= (1ull << 24)
                     ? (e->full_ions ? 2u : 3u)
                     : (per_source >= (1ull << 22) ? 2u : 0u);
  p.sigma_ref = 1.;
  if (e->full_ions) {
    double sigma_He;
    const ModelDev host_model = host_model_of(e);
    cmi_cross_sections_H_He(host_model, 1.0001 * e->model.nu_H, p.sigma_ref,
                            sigma_He);
  }
  p.source_bits = 0;
  /* (the continuous source counts as one more) */
  for (int s = e->model.nsource - (e->model.continuous_type != 0 ? 0 : 1);
       s > 0; s >>= 1)
    ++p.source_bits;
  if (p.source_bits > 10u - p.tau_bits)
    p.source_bits = 10u - p.tau_bits;
  p.dir_bits = 22u;
  if (tune.sort_dir_bits >= 0) {
    p.dir_bits = (uint32_t)tune.sort_dir_bits;
  } else {
    /* measured on 256^3, 1e8 packets: 21 bits order the packets as well as
     * 22 (20 nearly, 18 not), and 21 + 3 tau bits are three passes, not four */
    const uint32_t over = (22u + p.tau_bits + p.source_bits) % 8u;
    if (over == 1u || over == 2u)
      p.dir_bits = 22u - over;
  }
  p.key_bits = (int)(p.dir_bits + p.tau_bits + p.source_bits);
  /* the bucket order counts on uniform keys: the hydrogen-only ones are (the
   * Morton code of two uniform draws, the class from a third), the octaves of
   * a multi-ion packet's range are not; a block's selection and the key
   * kernel that writes the emission rows keep their own path */
  p.bucket_order = p.sorted && !p.select_mode && p.first != FIRST_PRE &&
                   !e->full_ions && tune.bucket_order;
  return CMI_GPU_OK;
}

/* the bucket order of a launch of n packets (take == 0: the radix sort) */
static BucketPlan bucket_plan_of(const cmi_gpu_engine *e, const LaunchPlan &p,
                                 uint64_t n) {
  if (!p.bucket_order) {
    BucketPlan none = {};
    return none;
  }
  return cmi_bucket_plan(n, p.key_bits, e->tune.bucket_bits1,
                         e->tune.bucket_bits2, e->tune.bucket_slack_permille,
                         e->tune.bucket_min_packets);
}

/* the buffers of a launch of at most `cap` flights */
static int reserve_for(cmi_gpu_engine *e, const LaunchPlan &p, uint64_t cap) {
  if (!e->span_cursor)
    HIP_TRY(hipMalloc(&e->span_cursor, sizeof(uint32_t) * CMI_SPAN_CURSORS));
  if (p.sorted || p.tiles)
    CMI_TRY(reserve_sort_buffers(e, cap, bucket_plan_of(e, p, cap).total_words));
  if (p.bucket_order && !e->bucket_meta)
    HIP_TRY(hipMalloc(&e->bucket_meta,
                      sizeof(uint32_t) * CMI_BUCKET_META_WORDS));
  if (p.passes)
    CMI_TRY(reserve_queues(e, cap));
  if (p.tiles)
    CMI_TRY(reserve_tile_buffers(e, cap));
  return CMI_GPU_OK;
}

/* workgroups of a transport launch over n flights: enough chunks for every
 * wave of a full grid, else fewer blocks */
static unsigned transport_blocks(const cmi_gpu_engine *e, uint64_t n,
                                 uint32_t chunk, int blocks_per_cu,
                                 int threads) {
  const uint64_t nchunks = (n + chunk - 1) / chunk;
  int64_t blocks = (int64_t)e->num_cu * blocks_per_cu;
  const int64_t need =
      (int64_t)((nchunks + (threads / 64) - 1) / (threads / 64));
  if (blocks > need)
    blocks = need;
  if (blocks < 1)
    blocks = 1;
  return (unsigned)blocks;
}

static QueueDev no_queue() {
  QueueDev q;
  memset(&q, 0, sizeof q);
  return q;
}

/* The escape tally's description on the device (cmi_escape_of) says "count"
 * exactly while the call's plan tracks: written, in stream order, when that
 * changes. */
static int publish_escape(cmi_gpu_engine *e, bool count) {
  count = count && e->escape.sky != nullptr;
  if (count == e->escape_counting)
    return CMI_GPU_OK;
  e->escape_staged = e->escape;
  if (!count)
    e->escape_staged.sky = nullptr;
  HIP_TRY(hipMemcpyAsync(cmi_escape_of(e->counters), &e->escape_staged,
                         sizeof(EscapeDev), hipMemcpyHostToDevice,
                         e->stream));
  /* (the copy may read its source after the call returns, and the next
   * change overwrites that source: wait - this happens twice per run) */
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->escape_counting = count;
  return CMI_GPU_OK;
}

/* the arguments of the first-generation launch over the ids [done, done +
 * nids) of a call, before the stages fill in what they decide */
static ShootArgs shoot_args(const cmi_gpu_engine *e, const LaunchPlan &p,
                            uint32_t seed, uint32_t iteration,
                            uint64_t first_packet, uint64_t done,
                            uint64_t nids, const double *flights) {
  ShootArgs a;
  a.grid = e->grid;
  a.model = e->model;
  a.cells = cells_of_iteration(e);
  a.counters = e->counters;
  a.first_packet = first_packet;
  a.batch_offset = done;
  a.n_packets = nids;
  a.order = nullptr;
  a.pre_rows = nullptr;
  a.xin = flights ? flights + (size_t)CMI_FLIGHT_DOUBLES * done : nullptr;
  a.xin_local = 0;
  a.xout.rows = e->export_rows;
  a.xout.count = e->export_count;
  a.xout.capacity = (unsigned int)e->export_capacity;
  a.pad_H = p.pad ? e->pad_H : nullptr;
  a.uniform_scale = p.uniform_scale;
  a.xcd_remap = (p.sorted && e->tune.xcd_remap) ? 1 : 0;
  a.pad_ny = e->grid.ncell[1] + 2 * CMI_PAD_LAYERS;
  a.pad_nz = e->grid.ncell[2] + 2 * CMI_PAD_LAYERS;
  a.pad_inv_yz = 1. / ((double)a.pad_ny * (double)a.pad_nz);
  a.pad_inv_z = 1. / (double)a.pad_nz;
  a.chunk = e->tune.chunk;
  a.seed = seed;
  a.iteration = iteration;
  /* handed-over flights are no ray bundles worth keeping together */
  a.refill_threshold = flights ? e->tune.refill_threshold_reemit
                               : e->tune.refill_threshold;
  a.exp_no_atomics = e->tune.exp_no_atomics;
  a.trackers = e->trackers;
  if (!p.tracking)
    a.trackers.n = 0;
  a.aggregate = flights ? p.agg_reemit : p.agg;
  a.qin = no_queue();
  a.qout = no_queue();
  a.park_in_place = 0;
  /* (launch_first_generation turns the claimed spans on) */
  a.span_cursor = nullptr;
  a.n_spans = 0;
  a.span_claim = 0;
  a.emit_before_flush = e->tune.emit_before_flush ? 1 : 0;
#ifdef CMI_EXPERIMENTS
  a.phase_clock = nullptr;
#endif
  return a;
}

/* the padded records of this call's cell state (0.1 ms at 256^3), unless
 * they are in place: the hydrogen-only update writes them with the records
 * (hydrogen_update_kernel), everything else that writes a record says so
 * (pad_records_stale) */
static int pad_records(cmi_gpu_engine *e, const LaunchPlan &p) {
  if (e->pad_valid)
    return CMI_GPU_OK;
  const GridDev &g = e->grid;
  if (!e->pad_H)
    HIP_TRY(hipMalloc(&e->pad_H, sizeof(double) * (size_t)p.padded_cells));
  pad_record_kernel<<<grid_blocks(e, p.padded_cells, 8), CMI_BLOCK, 0,
                      e->stream>>>(cells_of_iteration(e).opacity, e->pad_H,
                                   e->model.xsec_fixed[ION_H_n], g.ncell[0],
                                   g.ncell[1], g.ncell[2]);
  HIP_TRY(hipGetLastError());
  e->pad_valid = true;
  return CMI_GPU_OK;
}

/* A block of a decomposed grid: of the launch's a.n_packets ids, those that
 * start in the block (*select lists them, a.n_packets counts them). */
static int select_block_packets(cmi_gpu_engine *e, ShootArgs &a,
                                const uint32_t **select) {
  const uint64_t nids = a.n_packets;
  if (!e->select_count)
    HIP_TRY(hipMalloc(&e->select_count, sizeof(unsigned int)));
  CMI_TRY(grow(e, e->select_ids, e->select_capacity, nids,
               sizeof(uint32_t) * nids));
  HIP_TRY(hipMemsetAsync(e->select_count, 0, sizeof(unsigned int),
                         e->stream));
  SelectArgs sa;
  sa.grid = e->grid;
  sa.model = e->model;
  sa.first_packet = a.first_packet + a.batch_offset;
  sa.batch_offset = a.batch_offset;
  sa.n_packets = nids;
  sa.seed = a.seed;
  sa.iteration = a.iteration;
  sa.select = e->select_ids;
  sa.count = e->select_count;
  block_select_kernel<false>
      <<<grid_blocks(e, (int64_t)nids, 8), CMI_BLOCK, 0, e->stream>>>(sa);
  HIP_TRY(hipGetLastError());
  unsigned int mine = 0;
  CMI_TRY(read_counters(e, e->select_count, 1, &mine));
  a.n_packets = mine;
  *select = e->select_ids;
  return CMI_GPU_OK;
}

/* the queue the first generation parks its absorbed packets in */
static int open_ended_queue(cmi_gpu_engine *e, ShootArgs &a) {
  HIP_TRY(hipMemsetAsync(e->queue_counts, 0, 2 * sizeof(unsigned int),
                         e->stream));
  a.qout = e->ended_queue;
  if (!a.xin && e->tune.park_in_place) {
    /* new packets: parked at their place in the launch's order */
    a.park_in_place = 1;
    HIP_TRY(hipMemsetAsync(e->ended_queue.id, 0xff,
                           sizeof(uint32_t) * (size_t)a.n_packets, e->stream));
  }
  return CMI_GPU_OK;
}

/* keys and sort: a.order lists the launch's packets by source, direction and
 * tau class (and a.pre_rows holds their emission rows, FIRST_PRE); nids ids
 * in the launch, of which `select` (if not NULL) lists the a.n_packets that
 * fly */
enum OrderPath {
  ORDER_NONE = CMI_GPU_ORDER_NONE,
  ORDER_RADIX = CMI_GPU_ORDER_RADIX,
  ORDER_BUCKET = CMI_GPU_ORDER_BUCKET
};

/* the sort keys of a launch: nids ids, of which `select` (if not NULL) lists
 * the a.n_packets that fly; keys, ids and rows are the caller's to set */
static KeyArgs key_args(const cmi_gpu_engine *e, const LaunchPlan &p,
                        const ShootArgs &a, uint64_t nids,
                        const uint32_t *select) {
  const uint64_t n = a.n_packets;
  KeyArgs k;
  k.model = e->model;
  k.first_packet = a.first_packet + a.batch_offset;
  k.n_packets = n;
  k.seed = a.seed;
  k.iteration = a.iteration;
  k.tau_bits = p.tau_bits;
  /* (-1: the default of the branch that sets the class) */
  k.class_order =
      e->tune.class_order >= 0
          ? (uint32_t)e->tune.class_order
          : (e->full_ions ? CMI_CLASS_ORDER_FULL_DEFAULT
                          : CMI_CLASS_ORDER_DEFAULT);
  k.full_ions = e->full_ions ? 1 : 0;
  k.sigma_ref = p.sigma_ref;
  k.source_mask = (1u << p.source_bits) - 1u;
  /* coarse direction bins of ~64 x 2^tau_bits packets per source - or, tuning
   * "class_group_chunks", that many chunks of 64 per class */
  k.dir_hi_bits = 0;
  k.dir_bits = p.dir_bits;
  if (p.tau_bits != 0) {
    const uint64_t per_bin =
        (64ull * (uint64_t)e->tune.class_group_chunks) << p.tau_bits;
    /* (a block's own packets fill its part of the sphere as densely as
     * the launch's ids fill the whole) */
    const uint64_t per_source =
        nids / (uint64_t)(e->model.nsource > 0 ? e->model.nsource : 1);
    while (k.dir_hi_bits < p.dir_bits &&
           (per_source >> (k.dir_hi_bits + 1u)) >= per_bin)
      ++k.dir_hi_bits;
  }
  k.keys = nullptr;
  k.ids = nullptr;
  k.pre_rows = nullptr;
  k.select = select;
  return k;
}

/* The bucket order of a launch (packet_order.h): a.order lists its packets as
 * the radix sort would, with those that overflowed behind them. The regions,
 * the leaves and the order lie in the block of the sort buffers. */
static int order_packets_bucket(cmi_gpu_engine *e, const BucketPlan &bp,
                                const KeyArgs &k, ShootArgs &a) {
  uint32_t *block = e->sort_keys[0];
  uint32_t *meta = e->bucket_meta;
  BucketArgs b;
  b.n = (uint32_t)a.n_packets;
  b.key_bits = (uint32_t)(bp.bits1 + bp.bits2 + bp.rem_bits);
  b.bits1 = (uint32_t)bp.bits1;
  b.bits2 = (uint32_t)bp.bits2;
  b.rem_bits = (uint32_t)bp.rem_bits;
  b.region_cap = bp.region_cap;
  b.leaf_cap = bp.leaf_cap;
  b.order = block;
  b.regions = reinterpret_cast<uint2 *>(block + bp.region_begin);
  b.leaves = reinterpret_cast<uint2 *>(block + bp.leaf_begin);
  b.region_cursor = meta;
  b.leaf_cursor = meta + CMI_BUCKET_META_LEAF_CURSOR;
  b.overflow_cursor = meta + CMI_BUCKET_META_OVERFLOW;
  b.ordered = meta + CMI_BUCKET_META_ORDERED;
  b.leaf_offset = meta + CMI_BUCKET_META_LEAF_OFFSET;
  HIP_TRY(hipMemsetAsync(meta, 0, sizeof(uint32_t) * CMI_BUCKET_META_CLEARED,
                         e->stream));
  const uint32_t ntiles =
      (b.n + CMI_BUCKET_TILE - 1u) / CMI_BUCKET_TILE;
  int per_cu = 0;
  CMI_TRY(blocks_per_cu_of(bucket_key_kernel, CMI_BUCKET_THREADS, 8, per_cu));
  const uint32_t most = (uint32_t)(e->num_cu * per_cu);
  bucket_key_kernel<<<ntiles < most ? ntiles : most, CMI_BUCKET_THREADS, 0,
                      e->stream>>>(k, b);
  const uint32_t region_tiles =
      (b.region_cap + CMI_BUCKET_TILE - 1u) / CMI_BUCKET_TILE;
  bucket_split_kernel<<<dim3(region_tiles, 1u << b.bits1), CMI_BUCKET_THREADS,
                        0, e->stream>>>(b);
  const uint32_t nleaves = 1u << (b.bits1 + b.bits2);
  bucket_offsets_kernel<<<(nleaves + CMI_BUCKET_SCAN_THREADS - 1u) /
                              CMI_BUCKET_SCAN_THREADS,
                          CMI_BUCKET_SCAN_THREADS, 0, e->stream>>>(b);
  bucket_leaf_kernel<<<nleaves, CMI_BUCKET_LEAF_THREADS, 0, e->stream>>>(b);
  HIP_TRY(hipGetLastError());
  a.order = b.order;
  return CMI_GPU_OK;
}

/* keys and sort: a.order lists the launch's packets by source, direction and
 * tau class (and a.pre_rows holds their emission rows, FIRST_PRE); nids ids
 * in the launch, of which `select` (if not NULL) lists the a.n_packets that
 * fly */
static int order_packets(cmi_gpu_engine *e, const LaunchPlan &p, ShootArgs &a,
                         uint64_t nids, const uint32_t *select) {
  const uint64_t n = a.n_packets;
  KeyArgs k = key_args(e, p, a, nids, select);
  const BucketPlan bp = bucket_plan_of(e, p, n);
  /* (a launch whose plan needs more room than the block has - the buffers
   * were reserved for another plan - keeps the radix sort) */
  if (bp.take && !select && e->bucket_meta &&
      bp.total_words <= e->sort_block_words) {
    e->last_order_path = ORDER_BUCKET;
    e->last_bucket_bits[0] = bp.bits1;
    e->last_bucket_bits[1] = bp.bits2;
    return order_packets_bucket(e, bp, k, a);
  }
  e->last_order_path = ORDER_RADIX;
  k.keys = e->sort_keys[0];
  k.ids = e->sort_ids[0];
  k.pre_rows = p.first == FIRST_PRE ? e->tile_rows[1].weights : nullptr;
  if (p.first == FIRST_PRE && select) {
    /* the rows are addressed by packet id within the launch (that is what
     * the transport kernel knows): a block that flies a selection of the
     * ids needs room for all of them - the flight slots it borrows the
     * room from otherwise are sized for its selection */
    CMI_TRY(grow(e, e->select_rows, e->select_rows_capacity, nids,
                 sizeof(double) * CMI_NACC * (size_t)nids));
    k.pre_rows = e->select_rows;
  }
  a.pre_rows = k.pre_rows;
  if (k.pre_rows)
    emission_key_kernel<<<grid_blocks(e, (int64_t)n, 8), CMI_BLOCK, 0,
                          e->stream>>>(k);
  else
    direction_key_kernel<<<grid_blocks(e, (int64_t)n, 8), CMI_BLOCK, 0,
                           e->stream>>>(k);
  HIP_TRY(hipGetLastError());
  HIP_TRY(cmi_sort_pairs(e->sort_temp, e->sort_temp_bytes, e->sort_keys[0],
                         e->sort_keys[1], e->sort_ids[0], e->sort_ids[1], n,
                         p.key_bits, e->stream));
  a.order = e->sort_ids[1];
  return CMI_GPU_OK;
}

/* The block the point build's refill reads (PointEmitDev), for this launch:
 * written on the device, in stream order, ahead of EVERY launch of that
 * build - it holds the launch's seed, iteration, ids and order next to the
 * start of the source's flights, and the start cell's record as the cell
 * update before this launch left it. So there is no state of it to keep
 * valid: whatever a setter of sources, grid or records changed, the next
 * launch's block is made from what the engine then holds. (One thread, a few
 * microseconds a launch.) */
static int write_point_block(cmi_gpu_engine *e, const ShootArgs &a) {
  if (!e->point_emit)
    HIP_TRY(hipMalloc(&e->point_emit, sizeof(PointEmitDev)));
  PointEmitArgs s;
  memset(&s, 0, sizeof s);
  s.grid = a.grid;
  s.launch.first_packet = a.first_packet;
  s.launch.batch_offset = a.batch_offset;
  s.launch.order = a.order;
  s.launch.seed = a.seed;
  s.launch.iteration = a.iteration;
  s.launch.spectrum_type = a.model.spectrum_type;
  s.launch.mono_frequency = a.model.mono_frequency;
  s.launch.spectra = a.model.spectra;
  s.launch.spectrum_table = a.model.spectrum_table[0];
  s.launch.weight = a.model.photon_weight[0];
  s.source_position = a.model.source_position;
  s.pad_H = a.pad_H;
  s.pad_ny = a.pad_ny;
  s.pad_nz = a.pad_nz;
  s.out = e->point_emit;
  point_emit_kernel<<<1, 64, 0, e->stream>>>(s);
  HIP_TRY(hipGetLastError());
  return CMI_GPU_OK;
}

/* the first generation: one timed launch over the launch's flights */
static int launch_first_generation(cmi_gpu_engine *e, const LaunchPlan &p,
                                   const ShootArgs &args) {
  ShootArgs a = args;
  if (p.bundle_point)
    CMI_TRY(write_point_block(e, a));
  const unsigned blocks = transport_blocks(
      e, a.n_packets, a.chunk, p.blocks_per_cu_first, p.first_threads);
  if (e->tune.span_claim) {
    /* the cursors start at 0 in every launch (kernels without the
     * hydrogen-only block table do not look at them) */
    HIP_TRY(hipMemsetAsync(e->span_cursor, 0,
                           sizeof(uint32_t) * CMI_SPAN_CURSORS, e->stream));
    const uint64_t span = (uint64_t)(p.first_threads / 64) * a.chunk;
    a.span_cursor = e->span_cursor;
    a.n_spans = (uint32_t)((a.n_packets + span - 1) / span);
    a.span_claim = 1;
  }
#ifdef CMI_EXPERIMENTS
  if (e->tune.phase_stamps) {
    const size_t words = CMI_PHASE_COUNT + 1 + (size_t)blocks;
    if (e->phase_clock_capacity < words) {
      (void)hipFree(e->phase_clock);
      e->phase_clock = nullptr;
      e->phase_clock_capacity = 0;
      HIP_TRY(hipMalloc(&e->phase_clock, sizeof(unsigned long long) * words));
      e->phase_clock_capacity = words;
    }
    HIP_TRY(hipMemsetAsync(e->phase_clock, 0,
                           sizeof(unsigned long long) * words, e->stream));
    HIP_TRY(hipMemsetAsync(e->phase_clock + CMI_PHASE_COUNT, 0xff,
                           sizeof(unsigned long long), e->stream));
    e->phase_blocks = blocks;
    a.phase_clock = e->phase_clock;
  }
#endif
  EventPair kev;
  CMI_TRY(timer_begin(e, kev));
  if (p.bundle_point)
    p.kernel_point<<<blocks, p.first_threads, 0, e->stream>>>(a,
                                                              e->point_emit);
  else
    p.kernel_first<<<blocks, p.first_threads, 0, e->stream>>>(a);
  HIP_TRY(hipGetLastError());
  return timer_end(e, e->kernel_events, kev, a.n_packets);
}

/* what the interaction kernels of a launch have in common: they turn its
 * ended flights into new ones (everything else zero) */
static InteractArgs interact_args(const cmi_gpu_engine *e, const ShootArgs &a) {
  InteractArgs ia;
  memset(&ia, 0, sizeof ia);
  ia.model = e->model;
  ia.cells = cells_of_iteration(e);
  ia.counters = e->counters;
  ia.first_packet = a.first_packet;
  ia.seed = a.seed;
  ia.iteration = a.iteration;
  ia.qin = e->ended_queue;
  ia.grid = e->grid;
  return ia;
}

/* One timed pass of the transport kernel over `count` flights of a later
 * generation: the flights resume from `rows` (what the tile rounds left
 * over), or start from the ready queue (rows == NULL). Absorbed ones are
 * parked for the interaction kernel - except in the last pass, which follows
 * whatever is still re-emitted in place. */
static int launch_pass(cmi_gpu_engine *e, const LaunchPlan &p,
                       const ShootArgs &a, const double *rows,
                       unsigned int count, bool last) {
  ShootArgs b = a;
  b.park_in_place = 0;
  b.order = nullptr;
  b.xin = rows;
  b.xin_local = rows ? 1 : 0;
  b.n_packets = count;
  b.refill_threshold = e->tune.refill_threshold_reemit;
  b.aggregate = p.agg_reemit;
  b.qin = rows ? no_queue() : e->ready_queue;
  b.qout = last ? no_queue() : e->ended_queue;
  if (!last)
    HIP_TRY(hipMemsetAsync(e->ended_queue.count, 0, sizeof(unsigned int),
                           e->stream));
  const unsigned blocks = transport_blocks(
      e, count, b.chunk, last ? p.blocks_per_cu_inline : p.blocks_per_cu,
      CMI_BLOCK);
  EventPair gev;
  CMI_TRY(timer_begin(e, gev));
  (last ? p.kernel_inline : p.kernel)<<<blocks, CMI_BLOCK, 0, e->stream>>>(b);
  HIP_TRY(hipGetLastError());
  return timer_end(e, e->kernel_events, gev, count);
}

/* at most this many tile rounds per launch (what is left goes on as passes) */
#define CMI_TILE_MAX_ROUNDS 1000

/* The flights of a launch's tile rounds. By position (TileArgs): keys[i] and
 * the slot of position i < npos. Round 0: the slots as the interaction kernel
 * filled them, position = slot; every round writes the arrays of the next
 * one in its tile order, flights only - the rows never move, and what has
 * ended is gone from the arrays one round later. */
struct TileRounds {
  TileGridDev tg;
  int tile_bits; /* keys: tiles and the "free slot" key ntiles */
  uint32_t item_flights;
  bool defer;
  /* counters (cmi_gpu_engine::tile_counts) */
  unsigned int *d_nrows, *d_nlive, *d_nitems, *d_next, *d_new;
  InteractArgs ia;
  int cur; /* which set of rows holds the flights */
  FlightRowsDev rows;
  uint32_t *keys, *keys_next;
  const uint32_t *slot_of;
  int next_slot_of;
  unsigned int npos;
  /* slots the flights are spread over (since the last compaction) */
  unsigned int extent;
  /* of the round under way: its flights, its units of work, and the
   * positions in tile order */
  unsigned int nlive, nitems;
  const uint32_t *order;
};

/* the absorbed packets of the first generation -> flights in slots */
static int tile_rounds_begin(cmi_gpu_engine *e, const ShootArgs &a,
                             TileRounds &t) {
  t.tg = tile_grid(e);
  t.tile_bits = 1;
  while ((1ll << t.tile_bits) < (int64_t)t.tg.ntiles + 1)
    ++t.tile_bits;
  t.item_flights =
      e->full_ions ? CMI_TILE_ITEM_FLIGHTS_FULL : CMI_TILE_ITEM_FLIGHTS_H;
  t.defer = e->full_ions && e->tune.defer_weights;
  t.d_nrows = e->tile_counts;
  t.d_nlive = e->tile_counts + 1;
  t.d_nitems = e->tile_counts + 2;
  t.d_next = e->tile_counts + 3;
  t.d_new = e->tile_counts + 4;
  t.cur = 0;
  t.rows = e->tile_rows[t.cur];
  InteractArgs &ia = t.ia;
  ia = interact_args(e, a);
  ia.n_in = a.park_in_place ? (uint32_t)a.n_packets : 0u;
  ia.tiles = t.tg;
  ia.items = e->tile_items;
  ia.nitems = t.d_nitems;
  ia.absorbed_before = e->tile_absorbed_before;
  ia.ended_slot = e->tile_ended_slot;
  ia.new_slots = e->tile_new_slots;
  ia.new_count = t.d_new;
  ia.rows = t.rows;
  ia.rows.count = t.d_nrows;
  HIP_TRY(hipMemsetAsync(e->tile_counts, 0, 8 * sizeof(unsigned int),
                         e->stream));
  const int iblocks = e->num_cu * 8;
  if (t.defer)
    interaction_kernel<true, true, true>
        <<<iblocks, CMI_BLOCK, 0, e->stream>>>(ia);
  else if (e->full_ions)
    interaction_kernel<true, true><<<iblocks, CMI_BLOCK, 0, e->stream>>>(ia);
  else
    interaction_kernel<false, true><<<iblocks, CMI_BLOCK, 0, e->stream>>>(ia);
  HIP_TRY(hipGetLastError());
  unsigned int nslots = 0;
  CMI_TRY(read_counters(e, t.d_nrows, 1, &nslots));
  if (nslots > t.rows.capacity)
    return fail(CMI_GPU_ENOMEM,
                "tile rounds: %u flights, room for %u - flights were "
                "lost, the iteration is invalid",
                nslots, t.rows.capacity);
  if (t.defer && nslots != 0) {
    FlightWeightsArgs wa;
    wa.model = e->model;
    wa.rows = t.rows;
    wa.slots = nullptr;
    wa.count = nullptr;
    wa.n = nslots;
    flight_weights_kernel<<<grid_blocks(e, (int64_t)nslots, 8), CMI_BLOCK, 0,
                            e->stream>>>(wa);
    HIP_TRY(hipGetLastError());
  }
  t.keys = t.rows.keys;
  t.keys_next = e->tile_rows[1].keys;
  t.slot_of = nullptr;
  t.next_slot_of = 0;
  t.npos = nslots;
  t.extent = nslots;
  return CMI_GPU_OK;
}

/* the positions of a round in tile order (ended flights last), cut into units
 * of work: t.nlive flights in t.nitems units */
static int tile_round_order(cmi_gpu_engine *e, TileRounds &t) {
  TilePlanArgs pa;
  pa.tiles = t.tg;
  pa.sorted_keys = e->sort_keys[1];
  pa.nslots = t.npos;
  pa.tile_begin = e->tile_begin;
  pa.item_flights = t.item_flights;
  pa.items = e->tile_items;
  pa.nitems = t.d_nitems;
  pa.next_item = t.d_next;
  pa.nlive = t.d_nlive;
  if (e->tile_blockhist && e->tune.tile_counting_sort) {
    TileSortArgs sa;
    sa.keys = t.keys;
    sa.nslots = t.npos;
    sa.ntiles = (uint32_t)t.tg.ntiles;
    /* (about a counter per slot and workgroup at least) */
    {
      uint64_t nb = ((uint64_t)t.npos / sa.ntiles + 7) / 8 * 8;
      if (nb < 8)
        nb = 8;
      if (nb > CMI_TILE_SORT_BLOCKS)
        nb = CMI_TILE_SORT_BLOCKS;
      sa.nblocks = (uint32_t)nb;
    }
    sa.blockhist = e->tile_blockhist;
    sa.total = e->tile_total;
    sa.tile_begin = e->tile_begin;
    sa.order = e->sort_ids[1];
    tile_count_kernel<<<sa.nblocks, CMI_TILE_SORT_THREADS, 0, e->stream>>>(sa);
    tile_column_kernel<<<(sa.ntiles + CMI_BLOCK - 1) / CMI_BLOCK, CMI_BLOCK, 0,
                         e->stream>>>(sa);
    tile_offsets_kernel<<<1, CMI_TILE_SORT_THREADS, 0, e->stream>>>(sa);
    tile_scatter_kernel<<<sa.nblocks, CMI_TILE_SORT_THREADS, 0, e->stream>>>(
        sa);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(cmi_sort_pairs(e->sort_temp, e->sort_temp_bytes, t.keys,
                           e->sort_keys[1], e->tile_iota, e->sort_ids[1],
                           t.npos, t.tile_bits, e->stream));
    tile_begin_kernel<<<grid_blocks(e, (int64_t)t.npos + 1, 8), CMI_BLOCK, 0,
                        e->stream>>>(pa);
    HIP_TRY(hipGetLastError());
  }
  tile_plan_kernel<<<1, CMI_TILE_PLAN_THREADS, 0, e->stream>>>(pa);
  HIP_TRY(hipGetLastError());
  unsigned int plan[2] = {0, 0}; /* flights, units of work */
  CMI_TRY(read_counters(e, t.d_nlive, 2, plan));
  t.nlive = plan[0];
  t.nitems = plan[1];
  t.order = e->sort_ids[1];
  return CMI_GPU_OK;
}

/* the live rows into the other set of rows, in tile order: position j of
 * this round is then place j and slot j */
static int tile_round_compact(cmi_gpu_engine *e, TileRounds &t) {
  TileCompactArgs ca;
  ca.from = t.rows;
  ca.to = e->tile_rows[1 - t.cur];
  /* (the two key arrays change hands every round, whatever set of rows is in
   * use: the copies' keys go to the one that is free) */
  ca.to.keys = t.keys_next;
  ca.order = e->sort_ids[1];
  ca.slot_in = t.slot_of;
  ca.keys_in = t.keys;
  ca.nlive = t.d_nlive;
  ca.with_weights = e->full_ions ? 1 : 0;
  tile_compact_kernel<<<grid_blocks(e, 8ll * t.nlive, 8), CMI_BLOCK, 0,
                        e->stream>>>(ca);
  HIP_TRY(hipGetLastError());
  t.cur = 1 - t.cur;
  t.rows = e->tile_rows[t.cur];
  std::swap(t.keys, t.keys_next);
  t.slot_of = nullptr;
  t.order = e->tile_iota;
  t.extent = t.nlive;
  return CMI_GPU_OK;
}

/* the round itself: every flight through ONE tile, timed */
static int tile_round_launch(cmi_gpu_engine *e, const LaunchPlan &p,
                             const ShootArgs &a, const TileRounds &t) {
  TileArgs ta;
  ta.grid = e->grid;
  ta.model = e->model;
  ta.cells = cells_of_iteration(e);
  ta.counters = e->counters;
  ta.tiles = t.tg;
  ta.refill_threshold = e->tune.tile_refill_threshold;
  ta.rows = t.rows;
  ta.order = t.order;
  ta.slot_in = t.slot_of;
  ta.keys_out = t.keys_next;
  ta.slot_out = e->tile_slot_of[t.next_slot_of];
  ta.items = e->tile_items;
  ta.nitems = t.d_nitems;
  ta.next_item = t.d_next;
  ta.ended = e->ended_queue;
  ta.ended_slot = e->tile_ended_slot;
  ta.ended_pos = e->tile_ended_pos;
  ta.absorbed_count = e->tile_absorbed_count;
  ta.xout = a.xout;
  /* no more workgroups than units of work can exist */
  int64_t tb = (int64_t)e->num_cu * p.tile_blocks_per_cu;
  const int64_t most =
      (int64_t)t.tg.ntiles + (int64_t)t.nlive / t.item_flights + 1;
  if (tb > most)
    tb = most;
  EventPair tev;
  CMI_TRY(timer_begin(e, tev));
  p.tile_kernel<<<(unsigned)tb, p.tile_threads, 0, e->stream>>>(ta);
  HIP_TRY(hipGetLastError());
  CMI_TRY(timer_end(e, e->kernel_events, tev, t.nlive));
  ++e->tile_rounds_run;
  return CMI_GPU_OK;
}

/* the packets absorbed in a round: re-emitted into their slots, their new
 * keys at their positions of the next round */
static int tile_round_reemit(cmi_gpu_engine *e, TileRounds &t) {
  InteractArgs &ia = t.ia;
  ia.rows = t.rows;
  ia.ended_pos = e->tile_ended_pos;
  ia.key_out = t.keys_next;
  absorbed_scan_kernel<<<1, CMI_TILE_PLAN_THREADS, 0, e->stream>>>(
      t.d_nitems, e->tile_absorbed_count, e->tile_absorbed_before);
  HIP_TRY(hipGetLastError());
  /* (about a quarter of a round's flights are absorbed) */
  const int sblocks = grid_blocks(e, (int64_t)t.nlive / 2 + 1, 8);
  if (t.defer) {
    HIP_TRY(hipMemsetAsync(t.d_new, 0, sizeof(unsigned int), e->stream));
    interaction_slots_kernel<true, true>
        <<<sblocks, CMI_BLOCK, 0, e->stream>>>(ia);
    HIP_TRY(hipGetLastError());
    FlightWeightsArgs wa;
    wa.model = e->model;
    wa.rows = t.rows;
    wa.slots = e->tile_new_slots;
    wa.count = t.d_new;
    wa.n = 0;
    /* (about a tenth of a round's flights are re-emitted) */
    flight_weights_kernel<<<grid_blocks(e, (int64_t)t.nlive / 4 + 1, 8),
                            CMI_BLOCK, 0, e->stream>>>(wa);
  } else if (e->full_ions)
    interaction_slots_kernel<true><<<sblocks, CMI_BLOCK, 0, e->stream>>>(ia);
  else
    interaction_slots_kernel<false><<<sblocks, CMI_BLOCK, 0, e->stream>>>(ia);
  HIP_TRY(hipGetLastError());
  /* the next round: this round's places are its positions */
  std::swap(t.keys, t.keys_next);
  t.slot_of = e->tile_slot_of[t.next_slot_of];
  t.next_slot_of = 1 - t.next_slot_of;
  t.npos = t.nlive;
  return CMI_GPU_OK;
}

/* Later generations, in tile rounds (tile_kernels.h): the interaction
 * kernel turns the ended flights into flight rows keyed by the tile they
 * start in; every round sorts the rows by tile, flies each flight through
 * ONE tile with the tile's accumulators in LDS, and collects the flights
 * that go on (into another tile, or re-emitted) for the next round.
 * *handover, *handover_count: the flights the rounds leave over. */
static int run_tile_rounds(cmi_gpu_engine *e, const LaunchPlan &p,
                           const ShootArgs &a, const double **handover,
                           unsigned int *handover_count) {
  TileRounds t;
  CMI_TRY(tile_rounds_begin(e, a, t));
  const unsigned int compact_ratio =
      e->tune.tile_compact_ratio >= 0
          ? (unsigned int)e->tune.tile_compact_ratio
          : (e->full_ions ? 2u : 0u);
  for (int round = 0; t.npos != 0; ++round) {
    CMI_TRY(tile_round_order(e, t));
    if (t.nlive == 0)
      break;
    /* a unit of work costs a fixed ~10-20 us (tile records in, tile
     * accumulators out); measured on MI355X the round beats single
     * atomics while a unit has a few hundred flights to share that */
    const uint64_t per_item = e->tune.tile_min_per_item >= 0
                                  ? (uint64_t)e->tune.tile_min_per_item
                                  : 200u;
    const bool finish = t.nlive < e->tune.tile_min_flights ||
                        (uint64_t)t.nlive < per_item * t.nitems ||
                        round >= CMI_TILE_MAX_ROUNDS;
    if (finish || (compact_ratio != 0 && (uint64_t)compact_ratio * t.nlive <
                                             (uint64_t)t.extent))
      CMI_TRY(tile_round_compact(e, t));
    if (finish) {
      /* too few flights per tile for the LDS accumulators to pay: the
       * rest goes on as passes of the transport kernel, the first of which
       * resumes the flights from their (fresh, dense) rows */
      *handover = t.rows.rows;
      *handover_count = t.nlive;
      break;
    }
    CMI_TRY(tile_round_launch(e, p, a, t));
    CMI_TRY(tile_round_reemit(e, t));
  }
  return CMI_GPU_OK;
}

/* ... or as passes of the transport kernel: the interaction kernel turns
 * the ended flights of one launch into the ready flights of the next.
 * Those start all over the grid in random directions, so these launches
 * refill eagerly instead of keeping ray bundles together. */
static int run_passes(cmi_gpu_engine *e, const LaunchPlan &p,
                      const ShootArgs &a, const double *handover,
                      unsigned int handover_count) {
  if (handover_count != 0) {
    /* pass 0 of the tail: the flights resume from their slots, absorbed
     * ones are parked for the interaction kernel as in every pass */
    const bool last = handover_count < reemit_inline_below(e);
    CMI_TRY(launch_pass(e, p, a, handover, handover_count, last));
    if (last)
      handover_count = 0;
  }
  for (int gen = 0; p.passes && (!p.tiles || handover_count != 0); ++gen) {
    InteractArgs ia = interact_args(e, a);
    /* (the first pass reads what the first generation parked) */
    ia.n_in = (gen == 0 && !p.tiles && a.park_in_place)
                  ? (uint32_t)a.n_packets
                  : 0u;
    ia.qout = e->ready_queue;
    HIP_TRY(hipMemsetAsync(e->ready_queue.count, 0, sizeof(unsigned int),
                           e->stream));
    const int iblocks = e->num_cu * 8;
    if (e->full_ions)
      interaction_kernel<true, false><<<iblocks, CMI_BLOCK, 0, e->stream>>>(ia);
    else
      interaction_kernel<false, false>
          <<<iblocks, CMI_BLOCK, 0, e->stream>>>(ia);
    HIP_TRY(hipGetLastError());
    unsigned int count = 0;
    CMI_TRY(read_counters(e, e->ready_queue.count, 1, &count));
    if (count == 0)
      break;
    const bool last = count < reemit_inline_below(e) ||
                      gen + 2 >= e->tune.reemit_max_passes;
    CMI_TRY(launch_pass(e, p, a, nullptr, count, last));
    if (last)
      break;
  }
  return CMI_GPU_OK;
}

/* Transport of n_packets flights and of everything they re-emit: new packets
 * (flights == NULL) or flights handed over by other blocks of a decomposed
 * grid (device rows of CMI_FLIGHT_DOUBLES doubles). */
static int shoot_impl(cmi_gpu_engine *e, uint32_t seed, uint32_t iteration,
                      uint64_t first_packet, uint64_t n_packets,
                      const double *flights) {
  if (!e)
    return fail(CMI_GPU_EINVAL, "null engine");
  if (!e->have_sources || (e->model.nsource > 0 && !e->have_spectrum) ||
      (e->model.continuous_type != 0 && !e->have_continuous_spectrum) ||
      !e->have_xsec || !e->have_cells)
    return fail(CMI_GPU_ESTATE,
                "cmi_gpu_shoot: sources, their spectra, cross sections and "
                "cell data must be set first");
  if (n_packets == 0)
    return CMI_GPU_OK;
  /* (packet ids of a call are 32-bit, and 0xffffffff marks a place of the
   * ended queue that holds no flight: CMI_QUEUE_HOLE) */
  if (n_packets >= 0xffffffffull)
    return fail(CMI_GPU_EINVAL,
                "cmi_gpu_shoot: at most 2^32 - 2 packets per call");
  if (e->grid.decomposed &&
      (e->tune.exact_dda || !e->export_rows ||
       e->ncell >= CMI_FAST_MARCHER_MAX_CELLS))
    return fail(CMI_GPU_ESTATE,
                "cmi_gpu_shoot: a block of a decomposed grid needs an export "
                "buffer (cmi_gpu_set_export_buffer) and the incremental "
                "marcher (fewer than 2^28 cells per block)");
  if (!flights && e->grid.decomposed && block_emits_nothing(e))
    return CMI_GPU_OK;
  HIP_TRY(hipSetDevice(e->device));
  CMI_TRY(ensure_spectra(e));

  LaunchPlan plan;
  CMI_TRY(plan_launches(e, n_packets, flights, plan));
  if (!flights) { /* (for cmi_gpu_get_transport_plan) */
    e->last_first_build = (int32_t)plan.first;
    e->last_pad_uniform = plan.pad_uniform;
    e->last_bundle_march = plan.bundle;
    e->last_bundle_point = plan.bundle_point;
    if (!plan.sorted) /* (order_packets says which way otherwise) */
      e->last_order_path = ORDER_NONE;
  }
  CMI_TRY(publish_escape(e, plan.tracking));
  const uint64_t max_launch = e->tune.max_packets_per_launch;
  if (!plan.select_mode)
    CMI_TRY(reserve_for(e, plan, n_packets < max_launch ? n_packets
                                                         : max_launch));
  if (plan.pad)
    CMI_TRY(pad_records(e, plan));

  for (uint64_t done = 0; done < n_packets; done += max_launch) {
    /* the launch's packet ids ... */
    const uint64_t nids = n_packets - done < max_launch ? n_packets - done
                                                        : max_launch;
    ShootArgs a = shoot_args(e, plan, seed, iteration, first_packet, done,
                             nids, flights);
    /* ... and what it flies: all of them, or - a block of a decomposed grid -
     * those that start in the block */
    const uint32_t *select = nullptr;
    if (plan.select_mode) {
      CMI_TRY(select_block_packets(e, a, &select));
      if (a.n_packets == 0)
        continue;
      /* (some headroom: the count differs by a per cent from one iteration
       * to the next, and growing means freeing and allocating again) */
      CMI_TRY(reserve_for(e, plan, a.n_packets + a.n_packets / 16 + 1024));
    }
    if (plan.passes)
      CMI_TRY(open_ended_queue(e, a));

    EventPair ev;
    CMI_TRY(timer_begin(e, ev));
    if (plan.sorted)
      CMI_TRY(order_packets(e, plan, a, nids, select));
    CMI_TRY(launch_first_generation(e, plan, a));
    const double *handover = nullptr; /* flights the tile rounds leave over */
    unsigned int handover_count = 0;
    if (plan.tiles)
      CMI_TRY(run_tile_rounds(e, plan, a, &handover, &handover_count));
    CMI_TRY(run_passes(e, plan, a, handover, handover_count));
    CMI_TRY(timer_end(e, e->shoot_events, ev, 0));
  }
  return CMI_GPU_OK;
}

#endif /* CMI_TRANSPORT_DRIVER_H */
