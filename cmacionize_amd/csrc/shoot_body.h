/* The text of the transport kernels (kernels.h: shoot_kernel and
 * shoot_bundle_kernel include it as their body, with the flags FULL ... BIG
 * BUNDLE and POINT as constants in scope and the arguments as `a`). No include
 * guard: it is included once per kernel template. */
  static_assert(!POINT || (BUNDLE && SWITCH8),
                "POINT is a specialisation of the bundle build of one weight");
  static_assert(!BIG || PAD, "BIG: the padded march on large grids");
  static_assert(!BUNDLE || (PAD && !HEAT && !BIG),
                "BUNDLE is a specialisation of the padded march without the "
                "heating term, in the smaller blocks");
  constexpr int BLOCK = shoot_block_threads<FULL, TABLE, BIG>();
  /* (hydrogen-only table: slots = 2^TBITS) */
  constexpr int TBITS =
      (TABLE && !FULL)
          ? (BIG ? CMI_TABLE_BLOCK_BIG_BITS : CMI_TABLE_BLOCK_BITS)
          : CMI_TABLE_BITS;
  constexpr int TSLOTS = 1 << TBITS;
  /* PAD: the hydrogen-only first generation on a whole, non-periodic grid,
   * marching through the padded records (ShootArgs::pad_H) */
  static_assert(!PAD || (TABLE && !FULL && !REEMIT && !EXACT && !PRE),
                "PAD is a specialisation of the hydrogen-only TABLE kernel");
  constexpr bool TRACK = SWITCH8 && !PAD;
  static_assert(!TRACK || (!TABLE && !EXACT && !PRE),
                "TRACK is the tracker hook in the plain incremental marcher");
  /* UNIFORM: every packet of the launch carries one weight (plan_launches),
   * and one cross section as in every PAD kernel: the run sums and the table
   * add path lengths, and a slot's sum is multiplied by weight x sigma_H
   * (ShootArgs::uniform_scale) once, where it leaves the table */
  constexpr bool UNIFORM = SWITCH8 && PAD;
  static_assert(!UNIFORM || !HEAT,
                "the heating term's weight differs from packet to packet");
  const int lane = threadIdx.x & 63;
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  /* Blocks are dealt round-robin over the 8 XCDs (blocks b and b + 8 share
   * one - speed only, nothing depends on it): with xcd_remap the blocks of an
   * XCD take neighbouring positions of the sorted packet order, so that the
   * ray bundles flying through the same cells share one L2 */
  uint32_t block = blockIdx.x;
  if (a.xcd_remap) {
    const uint32_t xcd = block & 7u, q = gridDim.x >> 3, r = gridDim.x & 7u;
    block = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) +
            (block >> 3);
  }
  const uint64_t wave = (uint64_t)block * (BLOCK / 64) +
                        (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (BLOCK / 64);
  /* (BUNDLE: the plan takes it for chunks of 64 only) */
  const uint64_t chunk = BUNDLE ? 64 : a.chunk;

  /* wave-uniform cursor into the launch's position range */
  uint64_t chunk_begin = wave * chunk;
  uint64_t pos = chunk_begin;
  uint64_t pos_end = chunk_begin + chunk < a.n_packets ? chunk_begin + chunk
                                                       : a.n_packets;
  if (pos > pos_end)
    pos = pos_end;
  /* Claimed spans (ShootArgs::span_claim): the wave starts without positions;
   * the block takes spans of BLOCK / 64 chunks at the flush points, wave w
   * flies chunk w of a span - the waves of a block stay on one pencil. */
  constexpr bool CLAIM = TABLE && !FULL;
  const bool claim = CLAIM && (BUNDLE || a.span_claim != 0);
  __shared__ uint32_t s_span, s_span_part;
  if (claim) {
    chunk_begin = 0;
    pos = 0;
    pos_end = 0;
    if (threadIdx.x == 0) {
      s_span = CMI_SPAN_WANTED;
      s_span_part = a.xcd_remap ? (blockIdx.x & (CMI_SPAN_CURSORS - 1)) : 0u;
    }
  }
#ifdef CMI_EXPERIMENTS
  /* cycle stamps per section (the experiments build only) */
  unsigned long long phase_cycles[CMI_PHASE_COUNT] = {0, 0, 0, 0, 0};
  unsigned long long phase_stamp = 0;
  const bool stamps = CLAIM && a.phase_clock != nullptr;
  if (stamps) {
    phase_stamp = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0)
      atomicMin(a.phase_clock + CMI_PHASE_COUNT,
                (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
#define CMI_PHASE_MARK(section)                                               \
  do {                                                                        \
    if (stamps) {                                                             \
      const unsigned long long now = __builtin_amdgcn_s_memtime();            \
      phase_cycles[section] += now - phase_stamp;                             \
      phase_stamp = now;                                                      \
    }                                                                         \
  } while (0)
#else
#define CMI_PHASE_MARK(section)                                               \
  do {                                                                        \
  } while (0)
#endif

  Packet<FULL> p;
  /* Lanes without a packet take part in the cross-lane sums with a path
   * length of zero times their cross section / weights: those must be finite
   * (0 x NaN would poison the neighbours' sums), so nothing a sum multiplies
   * may start out as register or LDS garbage. */
  p.sigma_H = 0.;
  p.sigma_He_corr = 0.;
  p.nu = 0.;
  p.weight = 1.;
  PacketRng rng;
  /* (park_in_place launches: the packet's POSITION in the launch's order
   * instead - the id follows from it, id_of() below - so that parking at the
   * position costs no register across the march: a second value did cost the
   * hydrogen-only first generation, whose 64 are all taken, 0.3 of 34.6 ms,
   * and a build without the parking code, of all things, spilled the cross
   * section inside the march loop: 38.5 ms) */
  uint32_t packet_id = 0;
  auto id_of = [&](uint32_t held) -> uint32_t {
    return a.park_in_place
               ? (uint32_t)a.batch_offset + (a.order ? a.order[held] : held)
               : held;
  };
  uint32_t lane_meta = 0; /* rng position of the lane's packet (cmi_pack_meta) */
  bool active = false;
  int32_t last_cell = -1; /* EXACT marcher on grids >= 2^31 cells: see below */
  int64_t last_cell_wide = -1;

  /* packets finished per type (their weights are summed at the end:
   * src/IonizationPhotonShootJob.hpp:143-144); those that came from the
   * continuous source are counted a second time, per wave, in LDS */
  unsigned int tc0 = 0, tc1 = 0, tc2 = 0, tc3 = 0;
  /* BUNDLE: the same counts, of the wave, from two ballots over the lanes
   * whose flights a round ends. Without re-emission a packet ends as what it
   * was emitted as, TYPE_PRIMARY, or as TYPE_ABSORBED: the flights ended and
   * the absorbed ones among them are all there is to count, once for all
   * packets (s_ended) and once for those of the round's lanes whose packet the
   * continuous source emitted (s_continuous, as in the general build; the
   * lanes' mask is taken at the emission). The masks and their counts are
   * scalar; the running totals and the mask wait in the wave's own words of
   * LDS, written and read by its first lane: held in scalar registers across
   * the march they cost the build with a product per lane one scalar line of
   * every trip (a mask pair saved and restored around the axis advances). */
  __shared__ unsigned int s_ended[BLOCK / 64][2];
  __shared__ unsigned long long s_continuous_lanes[BLOCK / 64];
  if (BUNDLE && lane < 2)
    s_ended[threadIdx.x >> 6][lane] = 0;
  __shared__ unsigned int s_continuous[BLOCK / 64][4];
  if (lane < 4)
    s_continuous[threadIdx.x >> 6][lane] = 0;
  unsigned int nsteps = 0, natomics = 0; /* per lane and launch: < 2^32 */
  unsigned int nwavesteps = 0;
  /* PAD: the steps of the whole wave (wave-uniform: scalar arithmetic), and
   * the record of the cell the lane's packet is about to cross - it lives
   * across refills of other lanes, and says "outside" by itself */
  unsigned long long nsteps_wave = 0;
  double pad_next = CMI_PAD_GHOST;
  const bool any_periodic =
      !TABLE &&
      (a.grid.periodic[0] | a.grid.periodic[1] | a.grid.periodic[2]) != 0;
  const int aggregate = TABLE ? CMI_AGG_BLOCK : a.aggregate;

  /* H-only: per-wave write-combining cache in LDS. Scattered fp64 atomics
   * execute at the memory side at a chip-wide rate of a few 1e10 per second
   * whatever the schedule (measured: the kernel's time follows the number of
   * atomics, not the number of steps), so contributions are first combined on
   * chip: a run total goes into a direct-mapped table of (cell, partial sum)
   * with LDS atomics; only an entry that is evicted by another cell - or
   * flushed when the wave ends - costs a global atomic. A wave follows one
   * bundle of neighbouring rays, so consecutive steps (and the next bundle of
   * the wave's chunk) keep hitting the same few cells. The table is private to
   * the wave: no barriers, LDS operations of a wave execute in order. */
  /* CMI_AGG_BLOCK: per-block combining table. The 4 waves of a block follow
   * neighbouring ray bundles (consecutive positions of the sorted order), which
   * cross the same cells within a few steps of each other - too far apart in
   * time for the small wave cache, and a cache shared between waves cannot
   * evict safely without locks. So the table is insert-only: a run total
   * claims a slot for its cell with an LDS compare-and-swap (linear probing,
   * CMI_TABLE_PROBES tries, then it falls back to a global atomic) and adds
   * with ds_add_f64; between two bundles the block meets at a barrier and
   * flushes every used slot with ONE global atomic per cell. */
  /* (the multi-ion first generation sums cell by cell in registers and has
   * no table: accumulate_full_grouped) */
  constexpr bool GROUPED = FULL && TABLE;
  constexpr int lds_slots =
      GROUPED ? 1 : (FULL ? CMI_FTABLE_SLOTS : TSLOTS);
  constexpr int lds_values = FULL ? CMI_NACC : (HEAT ? 2 : 1);
  constexpr int TS = PAD ? CMI_PAD_TAG_STRIDE : 1;
  __shared__ int32_t lds_tag[TS * lds_slots];
  /* FULL: one more row, the sink of table_row() for lanes without a slot */
  __shared__ double lds_val[lds_values * (lds_slots + (FULL ? 1 : 0))];
  __shared__ int32_t block_has_work[BLOCK / 64];
  const int wib = threadIdx.x >> 6;
  /* FULL: per-wave accumulation weights and per-step scratch in LDS */
  __shared__ FullStage full_stage[FULL ? BLOCK / 64 : 1];
  FullStage &stage = full_stage[FULL ? wib : 0];
  double weights[CMI_NACC];
  double wq[CMI_NACC]; /* FULL: transposed weights of the lane's quarter */
  if (FULL) {
#pragma unroll
    for (int i = 0; i < CMI_NACC; ++i) {
      weights[i] = 0.;
      wq[i] = 0.;
      stage.weight[lane][i] = 0.;
    }
  }
  /* Multi-ion kernels use the same kind of table with 16 values per slot
   * (one accumulator row). 128 B per slot leave room for 256 slots only, so
   * the block writes it back every CMI_FTABLE_WINDOW iterations of the march
   * loop as well - the waves of a block advance together, one Manhattan shell
   * per iteration, so a cell's contributions arrive within a few iterations
   * of each other. */
  const bool use_table =
      !GROUPED && (TABLE || a.aggregate == CMI_AGG_BLOCK);
  if (use_table) {
    for (int k = threadIdx.x; k < lds_slots; k += BLOCK)
      lds_tag[TS * k] = -1;
    for (int k = threadIdx.x; k < lds_values * lds_slots; k += BLOCK)
      lds_val[k] = 0.;
    __syncthreads();
  }
  /* A flush point: every wave of the block arrives, the table is written
   * back with one global atomic per value, and all learn whether any wave has
   * work left. Waves may arrive from different places in the code - the
   * points are interchangeable - but every wave must keep arriving until the
   * block is done: a wave never exits while others may wait at a barrier. */
  /* Wave 0, before the barrier: the block's next span, unless it still holds
   * one no wave has taken. One lane asks the cursor of the block's XCD - and,
   * once that part of the spans is used up, the next XCD's; the answer goes
   * to LDS, where every wave reads it after the barrier. */
  auto claim_span = [&]() {
    if (__builtin_amdgcn_readfirstlane(s_span) != CMI_SPAN_WANTED)
      return;
    const uint32_t nparts = a.xcd_remap ? CMI_SPAN_CURSORS : 1u;
    const uint32_t q = a.xcd_remap ? a.n_spans / CMI_SPAN_CURSORS : a.n_spans;
    const uint32_t r = a.xcd_remap ? a.n_spans % CMI_SPAN_CURSORS : 0u;
    uint32_t part =
        __builtin_amdgcn_readfirstlane(s_span_part);
    uint32_t got = CMI_SPAN_NONE;
    for (uint32_t tried = 0; tried < nparts; ++tried) {
      const uint32_t begin = part * q + (part < r ? part : r);
      const uint32_t count = q + (part < r ? 1u : 0u);
      uint32_t v = 0;
      if (lane == 0)
        v = atomicAdd(a.span_cursor + part, 1u);
      v = __builtin_amdgcn_readfirstlane(v);
      if (v < count) {
        got = begin + v;
        break;
      }
      part = part + 1u == nparts ? 0u : part + 1u;
    }
    if (lane == 0) {
      s_span = got;
      s_span_part = part;
    }
  };
  auto flush_point = [&](bool has_work) -> bool {
    if (CLAIM && claim && __builtin_amdgcn_readfirstlane(wib) == 0)
      claim_span();
    /* (bit 1: the wave has used up its chunk) */
    if (lane == 0)
      block_has_work[wib] =
          (has_work ? 1 : 0) | ((CLAIM && claim && pos == pos_end) ? 2 : 0);
    CMI_PHASE_MARK(CMI_PHASE_END);
    __syncthreads();
    CMI_PHASE_MARK(CMI_PHASE_BARRIER);
    if (FULL) {
      const int i = threadIdx.x & 15;
      for (int k = threadIdx.x >> 4; k < lds_slots; k += BLOCK / 16) {
        const int32_t t = lds_tag[k];
        if (t >= 0) {
          /* (table rows are in column order, like the cells' rows) */
          if (HEAT || ((CMI_ACC_COLUMNS_OF_IONS >> i) & 1u) != 0u) {
            atomic_add_f64(a.cells.acc_base + (int64_t)t * CMI_NACC + i,
                           lds_val[k * CMI_NACC + i]);
            lds_val[k * CMI_NACC + i] = 0.;
            ++natomics;
          }
          if (i == 0)
            lds_tag[k] = -1; /* after the 16 lanes of the wave have read it */
        }
      }
    } else {
      for (int k = threadIdx.x; k < lds_slots; k += BLOCK) {
        const int32_t t = lds_tag[TS * k];
        /* (PAD: a record's byte offset, which may have bit 31 set) */
        if (PAD ? t != -1 : t >= 0) {
          const int32_t c =
              PAD ? cmi_unpad_cell(a, a.grid, cmi_pad_index(t)) : t;
          atomic_add_f64(acc_at(a.cells, ION_H_n, c),
                         UNIFORM ? lds_val[k] * a.uniform_scale : lds_val[k]);
          lds_val[k] = 0.;
          if (HEAT) {
            atomic_add_f64(acc_at(a.cells, CMI_NION, c),
                           lds_val[lds_slots + k]);
            lds_val[lds_slots + k] = 0.;
          }
          lds_tag[TS * k] = -1;
          natomics += HEAT ? 2 : 1;
        }
      }
    }
    int any_work = 0, all_waves = 2;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
      any_work |= block_has_work[w];
      all_waves &= block_has_work[w];
    }
    any_work &= 1;
    bool took = false;
    if (CLAIM && claim) {
      /* the span the block holds: once every wave has used up its chunk, wave
       * w takes chunk w of it (a short last span leaves some waves without
       * positions: they keep arriving here) */
      const uint32_t span =
          __builtin_amdgcn_readfirstlane(s_span);
      if (span != CMI_SPAN_NONE)
        any_work = 1;
      took = span != CMI_SPAN_NONE &&
             __builtin_amdgcn_readfirstlane(all_waves) != 0;
      if (took) {
        chunk_begin =
            ((uint64_t)span * (BLOCK / 64) +
             (uint64_t)__builtin_amdgcn_readfirstlane(wib)) *
            chunk;
        pos = chunk_begin < a.n_packets ? chunk_begin : a.n_packets;
        pos_end = chunk_begin + chunk < a.n_packets ? chunk_begin + chunk
                                                    : a.n_packets;
      }
    }
    __syncthreads();
    /* (after every wave has read it) */
    if (CLAIM && took && threadIdx.x == 0)
      s_span = CMI_SPAN_WANTED;
    CMI_PHASE_MARK(CMI_PHASE_FLUSH);
    return any_work != 0;
  };
  /* add (v0[, v1]) to `cell` through the block table, for the lanes given as
   * a mask (called by all 64 lanes): the search for a slot is kept as that
   * mask - `looking` loses the lanes that found theirs - and the probe loop's
   * exit is a scalar test */
  auto table_add_masked = [&](unsigned long long looking, int32_t cell,
                              double v0, double v1) {
    uint32_t slot;
    if (PAD) {
      /* (a full-rate 24-bit multiply - the cells of a bundle differ in their
       * low bits; asm: the compiler widens __umul24 to the quarter-rate
       * v_mul_lo_u32) */
      uint32_t product;
#if CMI_PAD_HASH_LOW_BITS > 0
      /* the low bits of the slot are the low bits of the padded index - z + 2 y
       * + 4 x modulo 8 with an even padded extent: the cells of a 2 x 2 x 2
       * neighbourhood, where the lanes of a bundle sit at any one step, fall
       * into different LDS banks -, the rest is hashed */
      const uint32_t index = (uint32_t)cmi_pad_index(cell);
      asm("v_mul_u32_u24 %0, 0x9e3779, %1"
          : "=v"(product)
          : "v"(index >> CMI_PAD_HASH_LOW_BITS));
      slot = (((product >> (24 - TBITS + CMI_PAD_HASH_LOW_BITS))
               << CMI_PAD_HASH_LOW_BITS) |
              (index & ((1u << CMI_PAD_HASH_LOW_BITS) - 1u))) &
             (TSLOTS - 1);
#else
      /* (`cell` is 8 x the padded index: the product's bits sit three places
       * up, and the multiply's 24 bits hold the index's low 21 - cells 2^21
       * apart in the padded index share a slot, no neighbours do) */
      asm("v_mul_u32_u24 %0, 0x9e3779, %1" : "=v"(product) : "v"(cell));
      slot = (product >> (24 - TBITS + 3)) & (TSLOTS - 1);
#endif
    } else {
      slot = ((uint32_t)cell * 0x9E3779B1u) >> (32 - TBITS);
    }
    for (int probe = 0; probe < CMI_TABLE_PROBES; ++probe) {
      /* (lanes that are not looking: whatever the register holds, they are
       * masked out below) */
      int32_t was;
      asm volatile("" : "=v"(was));
      unsigned long long found;
      if (CMI_TABLE_READ_FIRST) {
        if (lanes_of(looking))
          was = *(volatile int32_t *)&lds_tag[TS * slot];
        found = looking & mask_eq(was, cell);
        const unsigned long long vacant = looking & mask_eq(was, -1);
        if (vacant != 0ull) {
          int32_t got;
          asm volatile("" : "=v"(got));
          if (lanes_of(vacant))
            got = atomicCAS(&lds_tag[TS * slot], -1, cell);
          found |= vacant & (mask_eq(got, -1) | mask_eq(got, cell));
        }
      } else {
        if (lanes_of(looking))
          was = atomicCAS(&lds_tag[TS * slot], -1, cell);
        found = looking & (mask_eq(was, -1) | mask_eq(was, cell));
      }
      if (lanes_of(found)) {
        atomicAdd(&lds_val[slot], v0); /* ds_add_f64 */
        if (HEAT)
          atomicAdd(&lds_val[TSLOTS + slot], v1);
      }
      looking &= ~found;
      if (lanes_of(looking))
        slot = (slot + 1) & (TSLOTS - 1);
      if (looking == 0ull)
        return;
    }
    if (lanes_of(looking)) {
      const int32_t c =
          PAD ? cmi_unpad_cell(a, a.grid, cmi_pad_index(cell)) : cell;
      atomic_add_f64(acc_at(a.cells, ION_H_n, c),
                     UNIFORM ? v0 * a.uniform_scale : v0);
      if (HEAT)
        atomic_add_f64(acc_at(a.cells, CMI_NION, c), v1);
      natomics += HEAT ? 2 : 1;
    }
  };
  for (;;) {
    /* BUNDLE: a round ends every flight it began (the march below goes on
     * until no lane flies), so the refill finds a whole idle wave and nothing
     * of the last round's packets is read again */
    if (BUNDLE)
      active = false;
    /* POINT: the block the refill reads (PointEmitDev), through a pointer the
     * compiler learns anew every round - its loads stay in the refill, they
     * cannot be lifted above the march and their values kept across it */
    const __attribute__((address_space(4))) PointEmitDev *point_block = nullptr;
    if constexpr (POINT) {
      point_block =
          (const __attribute__((address_space(4))) PointEmitDev *)point;
      asm volatile("" : "+s"(point_block));
    }
    const unsigned long long active_mask = BUNDLE ? 0ull : __ballot(active);
    const unsigned long long idle_mask = ~active_mask;
    if (!claim && pos == pos_end &&
        chunk_begin + nwaves * chunk < a.n_packets) {
      /* current chunk used up: jump to this wave's next one */
      chunk_begin += nwaves * chunk;
      pos = chunk_begin;
      pos_end = chunk_begin + chunk < a.n_packets ? chunk_begin + chunk
                                                  : a.n_packets;
    }
    const bool refill_first = CLAIM && a.emit_before_flush != 0;
    const bool has_work = active_mask != 0ull || pos_end != pos;
    if (use_table) {
      /* between two bundles (a block that claims its spans takes the next
       * one here) */
      if (!refill_first && !flush_point(has_work))
        break;
    } else if (!has_work) {
      break;
    }
    const uint64_t avail = pos_end - pos;
    if (avail != 0 && idle_mask != 0ull &&
        (active_mask == 0ull || (int)__popcll(idle_mask) >= a.refill_threshold)) {
      const uint64_t rank = __popcll(idle_mask & lane_lt);
      if (!active && rank < avail) {
        const uint64_t i = pos + rank;
        bool mine = true;
        if (!BUNDLE && !PRE && a.xin != nullptr) {
          /* a flight handed over by another block of the grid */
#ifdef CMI_DBG_XIN_SLOTS
          const uint64_t row =
              (a.xin_local && a.xin_slots) ? (uint64_t)a.xin_slots[i] : i;
          const double *r = a.xin + (size_t)CMI_FLIGHT_DOUBLES * row;
#else
          const double *r = a.xin + (size_t)CMI_FLIGHT_DOUBLES * i;
#endif
          int64_t cell_global;
          unsigned long long idmeta;
          if (a.xin_local) {
            /* a slot of the tile rounds (tile_kernels.h) */
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
              p.pos[ax] = r[ax];
              p.dir[ax] = r[3 + ax];
              p.inv_dir[ax] = 1. / p.dir[ax];
              p.tmax[ax] = r[CMI_SLOT_TMAX + ax];
            }
            p.t = r[CMI_SLOT_T];
            p.tau = r[CMI_SLOT_TAU];
            p.nu = r[CMI_SLOT_NU];
            cell_global = (int64_t)(uint32_t)__double_as_longlong(
                r[CMI_SLOT_CELL]);
            idmeta = (unsigned long long)__double_as_longlong(
                r[CMI_SLOT_IDMETA]);
          } else {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
              p.pos[ax] = r[ax];
              p.dir[ax] = r[3 + ax];
              p.inv_dir[ax] = 1. / p.dir[ax];
              p.tmax[ax] = r[7 + ax];
            }
            p.t = r[6];
            p.tau = r[10];
            p.nu = r[11];
            cell_global = __double_as_longlong(r[12]);
            idmeta = (unsigned long long)__double_as_longlong(r[13]);
          }
          packet_id = (uint32_t)idmeta;
          lane_meta = (uint32_t)(idmeta >> 32);
          if (REEMIT)
            rng.resume(a.seed, a.iteration, a.first_packet + packet_id,
                       lane_meta & 0xffffffu, (lane_meta >> 24) & 1u);
          p.type = (int32_t)(lane_meta >> 28);
          p.weight = a.model.photon_weight[cmi_meta_origin(lane_meta)];
          set_cross_sections(a.model, p, weights);
          if (!EXACT) {
            if (a.xin_local)
              resume_flight_local(a.grid, p, (int32_t)cell_global);
            else
              resume_flight(a.grid, p, cell_global);
          }
        } else if (!BUNDLE && !PRE && a.qin.id != nullptr) {
          /* a ready flight: re-emitted by the interaction kernel */
          packet_id = a.qin.id[i];
          lane_meta = a.qin.meta[i];
          if (REEMIT)
            rng.resume(a.seed, a.iteration, a.first_packet + packet_id,
                       lane_meta & 0xffffffu, (lane_meta >> 24) & 1u);
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) {
            p.pos[ax] = a.qin.pos[ax][i];
            p.dir[ax] = a.qin.dir[ax][i];
            p.inv_dir[ax] = 1. / p.dir[ax];
          }
          p.type = (int32_t)(lane_meta >> 28);
          p.weight = a.model.photon_weight[cmi_meta_origin(lane_meta)];
          p.nu = a.qin.nu[i];
          p.tau = a.qin.tau[i];
          set_cross_sections(a.model, p, weights);
          start_flight<FULL, EXACT>(a.grid, p);
        } else if constexpr (POINT) {
          /* a new packet of the one discrete source: emit_geometry's discrete
           * branch (PacketOrigin::fixed: draws 0 and 1 are passed over) and
           * emit_physics, on the block's values. Where the flight starts is
           * the block's: per lane the direction, its reciprocals, and for
           * every axis the wall ahead - a select by the direction's sign and
           * start_flight's product - and the wall distance. */
          const auto *pe = point_block;
          const auto *order =
              (const __attribute__((address_space(1))) uint32_t *)pe->order;
          packet_id =
              (uint32_t)pe->batch_offset + (order ? order[i] : (uint32_t)i);
          rng.init(pe->seed, pe->iteration, pe->first_packet + packet_id);
          rng.skip_block();
          random_direction(p, rng);
          p.type = TYPE_PRIMARY;
          p.t = 0.;
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) {
            p.tmax[ax] = (p.dir[ax] > 0.)
                             ? pe->wall_hi[ax] * p.inv_dir[ax]
                             : ((p.dir[ax] < 0.)
                                    ? pe->wall_lo[ax] * p.inv_dir[ax]
                                    : DBL_MAX);
            p.tdelta[ax] = (p.dir[ax] != 0.)
                               ? pe->cellside[ax] * fabs(p.inv_dir[ax])
                               : 0.;
          }
          const int32_t sx = pe->stride_x, sy = pe->stride_y;
          p.cstep[0] = (p.dir[0] > 0.) ? sx : -sx;
          p.cstep[1] = (p.dir[1] > 0.) ? sy : -sy;
          p.cstep[2] = (p.dir[2] > 0.) ? 8 : -8;
          p.cell = pe->start_offset;
          pad_next = pe->start_record;
          /* (the frequency: the draws it takes are what the march needs of
           * it - the records carry the one cross section) */
          ModelDev source;
          source.spectrum_type = pe->spectrum_type;
          source.mono_frequency = pe->mono_frequency;
          source.spectra = pe->spectra;
          source.spectrum_table[0].x = pe->spectrum_table.x;
          source.spectrum_table[0].y = pe->spectrum_table.y;
          source.spectrum_table[0].n = pe->spectrum_table.n;
          source.spectrum_table[0].interpolation =
              pe->spectrum_table.interpolation;
          p.nu = sample_source_spectrum(source, rng, 0u);
          p.tau = -log(rng.next());
        } else {
          packet_id =
              (uint32_t)a.batch_offset + (a.order ? a.order[i] : (uint32_t)i);
          rng.init(a.seed, a.iteration, a.first_packet + packet_id);
          const uint32_t origin =
              emit_geometry<FULL, EXACT>(a.grid, a.model, rng, p);
          if (!BUNDLE && a.grid.decomposed) {
            /* a block flies the packets that start in it (block_owns_start;
             * the launch's positions may already be the block's own packets
             * only - block_select_kernel - and then all of them are) */
            int skipped = 0;
            bool in_block = true;
            mine = block_owns_start<FULL, EXACT>(a.grid, p, packet_id, skipped,
                                                 in_block);
            if (skipped != 0 && mine) {
              nsteps += skipped; /* they are DDA steps of the undivided run */
#pragma unroll
              for (int ax = 0; ax < 3; ++ax)
                p.rem[ax] = (p.dir[ax] > 0.)
                                ? a.grid.ncell[ax] - 1 - p.index[ax]
                                : p.index[ax];
              if (!in_block)
                p.rem[0] = -1;
              p.cell = (p.index[0] * a.grid.ncell[1] + p.index[1]) *
                           a.grid.ncell[2] +
                       p.index[2];
            }
          }
          if (PAD) {
            /* the padded long index and its strides (start_flight has set
             * index[], the signs and rem[0] < 0 for a start outside the box) */
            const int32_t sy = a.pad_nz, sx = a.pad_ny * a.pad_nz;
            /* (as byte offsets of the records: cmi_pad_index) */
            p.cstep[0] = 8 * ((p.dir[0] > 0.) ? sx : -sx);
            p.cstep[1] = 8 * ((p.dir[1] > 0.) ? sy : -sy);
            p.cstep[2] = (p.dir[2] > 0.) ? 8 : -8;
            const bool outside = fast_outside(p);
            const int32_t padded =
                outside ? 0
                        : ((p.index[0] + CMI_PAD_LAYERS) * a.pad_ny +
                           (p.index[1] + CMI_PAD_LAYERS)) *
                                  a.pad_nz +
                              (p.index[2] + CMI_PAD_LAYERS);
            p.cell = (int32_t)((uint32_t)padded << 3);
            pad_next = outside ? CMI_PAD_GHOST : a.pad_H[padded];
          }
          if (mine) {
            if (PRE)
              emit_physics_from_row<FULL>(
                  a.model, rng, p, weights, origin,
                  a.pre_rows + (size_t)CMI_NACC *
                                   (packet_id - (uint32_t)a.batch_offset));
            else
              emit_physics<FULL>(a.model, rng, p, weights, origin);
            lane_meta = cmi_pack_meta(rng.block, rng.have, 0, origin);
          }
          if (!BUNDLE && a.park_in_place)
            packet_id = (uint32_t)i; /* the position; the id: id_of() */
        }
        if (FULL) {
#pragma unroll
          for (int i = 0; i < CMI_NACC; ++i)
            stage.weight[lane][i] = weights[cmi_acc_of_column(i)];
        }
        active = mine;
        last_cell = -1;
        last_cell_wide = -1;
      }
      const uint64_t taken = __popcll(idle_mask);
      pos += taken < avail ? taken : avail;
    }
    /* (POINT: there is no continuous source) */
    if (BUNDLE && !POINT) {
      const unsigned long long continuous_lanes =
          wave_ballot(active && cmi_meta_origin(lane_meta) != 0);
      if (lane == 0)
        s_continuous_lanes[threadIdx.x >> 6] = continuous_lanes;
    }
    CMI_PHASE_MARK(CMI_PHASE_REFILL);
    /* emit_before_flush: the flush point after the refill, with what the wave
     * knew before it */
    if (CLAIM && refill_first && !flush_point(has_work))
      break;
    /* more positions left for this wave (in this or a later chunk)? (A wave
     * of a block that claims its spans flies what it has to the end once its
     * chunk is used up: the next span comes when all the block's waves are
     * through theirs.) */
    const uint64_t avail_after =
        (pos_end - pos) +
        (!claim && chunk_begin + nwaves * chunk < a.n_packets ? 1 : 0);

    /* ---- hot loop: only the march and the accumulation. It runs until so
     * few lanes are still in flight that the wave is due for a refill (or
     * none is); what happens to a packet at the end of its flight is decided
     * after the loop, for all finished lanes together. ---- */
    /* FAST: the record of the cell a lane is about to cross is loaded one
     * iteration ahead, so that the load overlaps the accumulation */
    int window = 0;
    if (FULL)
      load_quarter_weights(stage, wq);
    if constexpr (PAD) {
      /* The same loop on the padded records. What bounds it is instruction
       * issue - a SIMD issues one vector AND one scalar instruction per four
       * cycles, so the loop is as long as the larger of its two counts
       * (measured: trading vector selects for execution-mask arithmetic, 2
       * scalar instructions per vector one saved, gained nothing; neither did
       * a software pipeline with two record loads in flight, nor 8 waves per
       * SIMD - the loads are not what it waits for). So: no cell counters per
       * axis (the ghost record says "outside"), every tied axis advances by
       * selects, run sums over groups of 8 lanes, a 24-bit multiply for the
       * hash. */
      /* (the cross section itself is not in the loop: the records carry it,
       * cmi_pad_record) */
      double wsig = UNIFORM ? 0. : p.weight * p.sigma_H;
      double hw = HEAT ? wsig * (p.nu - a.model.nu_H) : 0.;
      /* (kept in registers: recomputing them costs a multiplication a step) */
      if (!UNIFORM)
        asm volatile("" : "+v"(wsig), "+v"(hw));
      /* Round 4: every condition of the loop is a wave mask in scalar
       * registers (mask_gt, mask_eq, lanes_of): which lanes step, which axes
       * advance, where runs end, who still looks for a slot. The loop's exit
       * is then a scalar branch (the compiler no longer treats the loop as
       * divergent and keeps its counters in scalar registers), the run sums
       * need three vector instructions per round (run_sums_masked), and
       * vacuum is the record -0.: sigma x -0. leaves the optical depth alone
       * without a max(), its sign bit says "do not accumulate". */
      const unsigned long long active_lanes = wave_ballot(active);
      /* the run key of a lane that does not accumulate: something no other
       * lane has. Not a multiple of 8, as the cells' keys - byte offsets -
       * are, and not the table's "empty" -1 either way. (Kept in a register
       * of its own: the compiler rebuilds it in every iteration otherwise;
       * `lane` itself is not needed inside the loop.) */
      int32_t not_lane = ~(lane << 3);
      asm volatile("" : "+v"(not_lane));
      /* the base of the records in a scalar register pair: the load is
       * global_load_dwordx2 v, v_offset, s[base], no 64-bit add per lane */
      const __attribute__((address_space(1))) char *pad_base =
          (const __attribute__((address_space(1))) char *)a.pad_H;
      asm volatile("" : "+s"(pad_base));
      /* a refill is due once this many lanes are idle (never, if the wave
       * has no positions left): the loop goes on while more than
       * 64 - idle_limit lanes step - one population count serves the test
       * and the step counter, and "no lane steps" is the same test */
      const int idle_limit = __builtin_amdgcn_readfirstlane(
          avail_after != 0 ? a.refill_threshold : 65);
      /* (BUNDLE: the threshold is 64, the round flies until no lane does) */
      const int fly_min =
          BUNDLE ? 0 : (idle_limit < 64 ? 64 - idle_limit : 0);
      int zero = 0;
      asm volatile("" : "+v"(zero)); /* one register for the whole loop */
      const RunMasks pad_run_masks = run_masks<CMI_PAD_SCAN_ROUNDS>();
      unsigned int bundle_steps = 0; /* wave-uniform: a scalar register */
      /* the lanes' steps of this bundle (at most 64 per iteration: 32 bits
       * hold 6.7e7 iterations, a bundle has thousands) */
      unsigned int bundle_lane_steps = 0;
      /* the lanes whose packet has optical depth left, and of those the ones
       * inside the grid: they step. The loop is tested at its bottom - one
       * compare and one branch back, no exit flag. */
      unsigned long long in_flight = active_lanes & mask_gt(p.tau, 0.);
      unsigned long long flying = in_flight & mask_gt(pad_next, -1.5);
      int nflying = (int)__popcll(flying);
      if (nflying > fly_min) do {
        ++bundle_steps;
        bundle_lane_steps += (unsigned int)nflying;
        const bool stepping = lanes_of(flying);
        /* number density > 0: the record's sign bit is clear */
        const unsigned long long accumulating =
            flying & mask_ge(__double2hiint(pad_next), 0);
        /* the run key - the cell about to be crossed, or something no other
         * lane has - before the march moves on (this IS the copy of the old
         * cell index the accumulation needs) */
        /* (the smaller of two walls for every lane, stepping or not, next to
         * the key's compare and select: inside the branch of the stepping
         * lanes nothing is there to fill the wait state between the two
         * dependent minima, and it cost a no-op on the scalar side) */
        double t12 = min_f64(p.tmax[1], p.tmax[2]);
        int32_t key = lanes_of(accumulating) ? p.cell : not_lane;
        /* (here, not after the march: that would take a copy of the cell) */
        asm volatile("" : "+v"(key), "+v"(t12));
        /* (lanes that do not step take part in the run sums with a key of
         * their own and are never a tail that adds: their path length may be
         * anything, run_sums_masked selects, it does not multiply) */
        double ds;
        asm volatile("" : "=v"(ds));
        if (stepping) {
          const double tmin = min_f64(p.tmax[0], t12);
          const double t_old = p.t;
          ds = tmin - t_old;
          /* sigma n x_H of the cell: the record as it stands */
          const double sk = pad_next;
          p.tau -= ds * sk;
          /* every tied axis advances, under the execution mask: one add each
           * for the wall parameter and the cell (vector instructions are what
           * the loop is short of). The three masks are chained: one save and
           * one restore of the execution mask for all of them. */
          {
            unsigned long long saved;
            asm volatile("s_and_saveexec_b64 %[saved], %[m0]\n\t"
                         "v_add_f64 %[t0], %[t0], %[d0]\n\t"
                         "v_add_u32 %[cell], %[cell], %[c0]\n\t"
                         "s_and_b64 exec, %[saved], %[m1]\n\t"
                         "v_add_f64 %[t1], %[t1], %[d1]\n\t"
                         "v_add_u32 %[cell], %[cell], %[c1]\n\t"
                         "s_and_b64 exec, %[saved], %[m2]\n\t"
                         "v_add_f64 %[t2], %[t2], %[d2]\n\t"
                         "v_add_u32 %[cell], %[cell], %[c2]\n\t"
                         "s_mov_b64 exec, %[saved]"
                         : [t0] "+v"(p.tmax[0]), [t1] "+v"(p.tmax[1]),
                           [t2] "+v"(p.tmax[2]), [cell] "+v"(p.cell),
                           [saved] "=&s"(saved)
                         : [m0] "s"(mask_eq(p.tmax[0], tmin)),
                           [m1] "s"(mask_eq(p.tmax[1], tmin)),
                           [m2] "s"(mask_eq(p.tmax[2], tmin)),
                           [d0] "v"(p.tdelta[0]), [d1] "v"(p.tdelta[1]),
                           [d2] "v"(p.tdelta[2]), [c0] "v"(p.cstep[0]),
                           [c1] "v"(p.cstep[1]), [c2] "v"(p.cstep[2])
                         : "scc");
          }
          p.t = tmin;
          if (!(p.tau > 0.)) {
            /* the flight ends in this cell (a cell with gas - vacuum leaves
             * the optical depth alone -, so the key is the cell) */
            last_cell = key;
            if (p.tau < 0.) {
              /* Scorr = ds tau / tau_cell = tau / (sigma n x_H): reciprocal,
               * one Newton step, the quotient and its correction (~1e-16) */
              double r = __builtin_amdgcn_rcp(sk);
              r = __fma_rn(__fma_rn(-sk, r, 1.), r, r);
              double corr = p.tau * r;
              corr = __fma_rn(__fma_rn(-corr, sk, p.tau), r, corr);
              ds += corr;
              p.t = t_old + ds;
            }
          }
          /* the record of the next cell, for every lane that stepped. (A
           * lane whose flight has just ended inside the cell loads one too -
           * its neighbour's, a valid padded index -: nothing reads it, and
           * the compare, the mask and the branch that kept it from loading
           * cost every iteration.) */
          pad_next = *reinterpret_cast<
              const __attribute__((address_space(1))) double *>(
              pad_base + (uint32_t)p.cell);
        }
        /* whose packet has optical depth left: the head test of the next
         * iteration. (Outside the branch of the stepping lanes: a mask formed
         * inside it is a per-lane value to the compiler, and all the loop's
         * scalar bookkeeping with it.) */
        in_flight = flying & mask_gt(p.tau, 0.);
        if (CMI_EXP(a) == 12) {
          /* experiment: the march alone (results are wrong) */
          asm volatile("" ::"v"(ds), "s"(accumulating));
          continue;
        }
        /* (UNIFORM: the path length; its weight comes at the flush) */
        double v[2] = {UNIFORM ? ds : ds * wsig, HEAT ? ds * hw : 0.};
        /* run sums over groups of 2^rounds lanes (measured at 8 waves/SIMD
         * in round 3, ms per iteration of 1e8 packets: groups of 4 44.2,
         * groups of 8 43.0, groups of 16 44.6) */
        unsigned long long tails;
        if (HEAT)
          run_sums_masked<2, CMI_PAD_SCAN_ROUNDS>(key, v, tails, zero,
                                                  pad_run_masks);
        else
          run_sums_masked<1, CMI_PAD_SCAN_ROUNDS>(
              key, reinterpret_cast<double(&)[1]>(v), tails, zero,
              pad_run_masks);
        if (CMI_EXP(a) == 11) {
          /* experiment: no table (results are wrong) */
          asm volatile("" ::"v"(v[0]), "s"(tails));
          continue;
        }
        table_add_masked(tails & accumulating, key, v[0], v[1]);
      } while ((flying = in_flight & mask_gt(pad_next, -1.5),
                nflying = (int)__popcll(flying), nflying > fly_min));
      nwavesteps += bundle_steps;
      nsteps_wave += bundle_lane_steps;
      /* the rest of the kernel reads the flight's end the usual way */
      if (active && !(p.tau > 0. && pad_next > -1.5)) {
        p.rem[0] = (p.tau >= 0. && !(pad_next > -1.5)) ? -1 : 0;
        p.rem[1] = 0;
        p.rem[2] = 0;
        /* (a byte offset, which may have bit 31 set, or still -1) */
        /* (BUNDLE reads no more of it than "a cell was crossed": any cell) */
        if (last_cell != -1)
          last_cell =
              BUNDLE ? 0 : cmi_unpad_cell(a, a.grid, cmi_pad_index(last_cell));
      }
    }
    double2 kappa_next = make_double2(0., 0.);
    if (!PAD && !EXACT && active && p.tau > 0. && !fast_outside(p))
      kappa_next = fast_load_record(a.cells.opacity, p);
    /* (round 4: the lanes in flight as a scalar mask straight from the
     * compares, the refill test on scalars - see the PAD loop) */
    const unsigned long long active_lanes = wave_ballot(active);
    const int idle_limit = __builtin_amdgcn_readfirstlane(
        avail_after != 0 ? a.refill_threshold : 65);
    const RunMasks table_run_masks = run_masks<CMI_TABLE_SCAN_ROUNDS>();
    for (; !PAD;) {
      unsigned long long flying;
      if (EXACT)
        flying = wave_ballot(active && p.tau > 0. && is_inside(a.grid, p));
      else
        flying = active_lanes & mask_gt(p.tau, 0.) &
                 mask_ge(p.rem[0] | p.rem[1] | p.rem[2], 0);
      if (flying == 0ull || (int)__popcll(~flying) >= idle_limit)
        break;
      const bool stepping = lanes_of(flying);
      ++nwavesteps;
      double ds = 0.;
      bool accumulate = false;
      if (stepping) {
        double2 kappa;
        if (EXACT) {
          ds = dda_step(a.grid, a.cells.opacity, p, last_cell_wide, kappa);
          last_cell = (int32_t)last_cell_wide;
        } else {
          kappa = kappa_next;
          ds = fast_step(p, last_cell, kappa);
        }
        ++nsteps;
        accumulate = (kappa.x >= 0.); /* number density > 0 */
        /* DensityGrid::update_integrals' tracker hook,
         * src/DensityGrid.hpp:188-191 (SpectrumTracker::count_photon), and
         * DensitySubGrid::update_intensity_counters',
         * src/DensitySubGrid.hpp:614-617 (AbsorptionTracker::count_photon).
         * In the kernels of the exact marcher and in the TRACK builds of the
         * incremental one (blocks of a decomposed grid while trackers count:
         * in the other builds the hook's registers would spill the march
         * loop). */
        if ((EXACT || TRACK) && a.trackers.n != 0 && accumulate) {
          const int64_t tracked_cell =
              EXACT ? last_cell_wide : (int64_t)last_cell;
          for (int k = 0; k < a.trackers.n; ++k) {
            if (tracked_cell != a.trackers.cell[k])
              continue;
            if (a.trackers.kind[k] == CMI_TRACKER_ABSORPTION) {
              /* src/AbsorptionTracker.hpp:133-138: the step's contribution
               * to every mean intensity, by photon type */
              double *bins = a.trackers.absorption +
                             ((size_t)k * 4 + (size_t)p.type) * CMI_NION;
              const double dsw = ds * p.weight;
              if (FULL) {
                for (int ion = 0; ion < CMI_NION; ++ion)
                  atomic_add_f64(bins + ion,
                                 dsw * stage.weight[lane][cmi_acc_column(ion)]);
              } else {
                atomic_add_f64(bins + ION_H_n, dsw * p.sigma_H);
              }
              continue;
            }
            if (a.trackers.kind[k] == CMI_TRACKER_WEIGHTED) {
              /* src/WeightedSpectrumTracker.hpp:300-319: one over the area
               * the cell shows the packet, by photon type and frequency bin */
              const double direction[3] = {p.dir[0], p.dir[1], p.dir[2]};
              atomic_add_f64(
                  a.trackers.flux + 4 * (size_t)a.trackers.first_bin[k] +
                      (size_t)p.type * (size_t)a.trackers.nbins[k] +
                      (size_t)cmi_frequency_bin(a.trackers, k, p.nu),
                  1. / cmi_projected_area(direction));
              continue;
            }
            const double *d = a.trackers.direction[k];
            if (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] > 0. &&
                p.dir[0] * d[0] + p.dir[1] * d[1] + p.dir[2] * d[2] <
                    a.trackers.cos_opening_angle[k])
              continue;
            const uint32_t bin =
                (uint32_t)((p.nu - a.trackers.minimum_frequency) *
                           a.trackers.inverse_frequency_width[k]);
            if (bin < (uint32_t)a.trackers.nbins[k] && p.type < TYPE_ABSORBED)
              atomicAdd(a.trackers.counts +
                            3 * (size_t)a.trackers.first_bin[k] +
                            (size_t)p.type * (size_t)a.trackers.nbins[k] + bin,
                        1ull);
          }
        }
      }
      if (!EXACT && any_periodic && stepping && p.tau >= 0.)
        fast_wrap(a.grid, p);
      if (!EXACT && stepping && p.tau > 0. && !fast_outside(p))
        kappa_next = fast_load_record(a.cells.opacity, p);
      if (CMI_EXP(a) == 1)
        continue;
      if (GROUPED) {
        accumulate_full_grouped<HEAT>(
            a, wq, CMI_EXP(a) == 4 ? 0ull : wave_ballot(accumulate), last_cell,
            ds * p.weight, natomics);
      } else if (FULL) {
        accumulate_full<HEAT>(a, wq, accumulate, last_cell, ds * p.weight,
                              natomics, use_table ? lds_tag : nullptr,
                              lds_val);
        if (use_table && CMI_EXP(a) != 5 &&
            ++window == CMI_FTABLE_WINDOW) {
          window = 0;
          (void)flush_point(true);
        }
      } else if (aggregate != CMI_AGG_NONE) {
        /* lanes in the same cell: one add for the whole run */
        const int32_t key = accumulate ? last_cell : ~lane;
        const double dsw = accumulate ? ds * p.weight : 0.;
        bool tail;
        double v[2] = {dsw * p.sigma_H,
                       HEAT ? dsw * p.sigma_H * (p.nu - a.model.nu_H) : 0.};
        if (use_table) {
          /* the table merges equal cells anyway: sums over groups of 2^ROUNDS
           * lanes are enough to keep the LDS atomics few */
          unsigned long long tails;
          int zero = 0;
          asm volatile("" : "+v"(zero));
          if (HEAT)
            run_sums_masked<2, CMI_TABLE_SCAN_ROUNDS>(key, v, tails, zero,
                                                      table_run_masks);
          else
            run_sums_masked<1, CMI_TABLE_SCAN_ROUNDS>(
                key, reinterpret_cast<double(&)[1]>(v), tails, zero,
                table_run_masks);
          table_add_masked(tails & wave_ballot(accumulate), last_cell, v[0],
                           v[1]);
          continue;
        }
        if (HEAT)
          run_sums<2, 6>(key, v, tail);
        else
          run_sums<1, 6>(key, reinterpret_cast<double(&)[1]>(v), tail);
        const bool add = tail && accumulate;
        if (add) {
          atomic_add_f64(acc_at(a.cells, ION_H_n, last_cell), v[0]);
          if (HEAT)
            atomic_add_f64(acc_at(a.cells, CMI_NION, last_cell), v[1]);
          natomics += HEAT ? 2 : 1;
        }
      } else if (accumulate) {
        const int64_t c = EXACT ? last_cell_wide : (int64_t)last_cell;
        update_integrals_H<HEAT>(a, p.sigma_H, p.nu, p.weight, c, ds);
        natomics += HEAT ? 2 : 1;
      }
    }

    CMI_PHASE_MARK(CMI_PHASE_MARCH);
    /* ---- end of flight for every lane that cannot step any more ---- */
    int32_t ended_type = -1; /* BUNDLE: the type the lane's flight ended as */
    if (active) {
      bool inside_now;
      if (EXACT)
        inside_now = is_inside(a.grid, p);
      else
        inside_now = (p.tau < 0.) || !fast_outside(p);
      const int64_t cell_now = EXACT ? last_cell_wide : (int64_t)last_cell;
      if (!(inside_now && p.tau > 0.)) {
        bool absorbed = false, done = false;
        if (p.tau < 0.) {
          /* absorbed inside last_cell (the packet is still inside the box) */
          absorbed = true;
        } else if (inside_now) {
          /* tau hit 0 exactly on a wall, packet still inside: interact()
           * returns the last traversed cell */
          absorbed = (cell_now >= 0);
          done = !absorbed;
        } else {
          done = true; /* left the box: DensityGrid::end() */
          if (!BUNDLE && !EXACT && a.grid.decomposed &&
              (PAD || last_cell >= 0)) {
            /* ... or only this block of it: hand the flight over. (PAD: the
             * ghost cell the packet stands in says where it went; a packet
             * that never entered the block stands in the corner ghost cell
             * of padded index 0, which belongs to no block.) */
            int64_t cell_global;
            if constexpr (PAD)
              cell_global = pad_next > -1.5
                                ? -1
                                : exit_cell_global_padded(a, a.grid, p);
            else
              cell_global = exit_cell_global(a.grid, p, last_cell);
            if (cell_global >= 0) {
              const unsigned long long leaving = __ballot(true);
              unsigned int base = 0;
              const int first = __ffsll((long long)leaving) - 1;
              if (lane == first)
                base = atomicAdd(a.xout.count,
                                 (unsigned int)__popcll(leaving));
              base = __shfl(base, first, 64);
              const unsigned int q = base + __popcll(leaving & lane_lt);
              if (q < a.xout.capacity) {
                double *r = a.xout.rows + (size_t)CMI_FLIGHT_DOUBLES * q;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                  r[ax] = p.pos[ax];
                  r[3 + ax] = p.dir[ax];
                  r[7 + ax] = p.tmax[ax];
                }
                r[6] = p.t;
                r[10] = p.tau;
                r[11] = p.nu;
                r[12] = __longlong_as_double(cell_global);
                const uint32_t meta =
                    REEMIT
                        ? cmi_pack_meta(rng.block, rng.have, (uint32_t)p.type,
                                        cmi_meta_origin(lane_meta))
                        : ((lane_meta & CMI_META_KEEP_MASK) |
                           ((uint32_t)p.type << 28));
                r[13] = __longlong_as_double((long long)(
                    ((unsigned long long)meta << 32) | id_of(packet_id)));
                r[14] = 0.;
                r[15] = 0.;
              }
              done = false;
              active = false; /* continues in another block */
            }
          }
          /* the escape tally: the packet has left the WHOLE box (no hand-over,
           * and a periodic face is never left). One fp64 atomic in a packet's
           * life; in the builds with the trackers' hook only. (The tally's
           * description lives behind the counters, not in the arguments: see
           * cmi_escape_of.) */
          if constexpr (EXACT || TRACK) {
            const EscapeDev &s = *cmi_escape_of(a.counters);
            if (done && s.sky != nullptr && p.type < TYPE_ABSORBED) {
              const double direction[3] = {p.dir[0], p.dir[1], p.dir[2]};
              const int32_t bin = cmi_frequency_bin_of(
                  s.bins_type, s.nfreq, s.bins_min, s.bins_max,
                  s.inverse_frequency_width, s.level_edges, p.nu);
              atomic_add_f64(
                  s.sky +
                      ((size_t)p.type * (size_t)s.nfreq + (size_t)bin) *
                          ((size_t)s.nlon * (size_t)s.nmu) +
                      (size_t)cmi_escape_pixel(s.frame, s.nlon, s.nmu,
                                               direction),
                  p.weight);
            }
          }
        }
        if (!BUNDLE && absorbed && a.qout.id != nullptr) {
          /* park the packet for the interaction kernel (PhotonSource::reemit
           * happens there): wave-level compaction into the queue */
          if (!EXACT)
            end_flight(p); /* position of the absorption */
          unsigned int q = packet_id; /* park_in_place: the position */
          if (!a.park_in_place) {
            const unsigned long long parked = __ballot(true);
            unsigned int base = 0;
            const int first = __ffsll((long long)parked) - 1;
            if (lane == first)
              base = atomicAdd(a.qout.count, (unsigned int)__popcll(parked));
            base = __shfl(base, first, 64);
            q = base + __popcll(parked & lane_lt);
          }
#pragma unroll
          for (int ax = 0; ax < 3; ++ax)
            a.qout.pos[ax][q] = p.pos[ax];
          a.qout.nu[q] = p.nu;
          a.qout.cell[q] = (int32_t)cell_now;
          a.qout.id[q] = id_of(packet_id);
          a.qout.meta[q] =
              REEMIT ? cmi_pack_meta(rng.block, rng.have, (uint32_t)p.type,
                                     cmi_meta_origin(lane_meta))
                     : ((lane_meta & CMI_META_KEEP_MASK) |
                        ((uint32_t)p.type << 28));
          active = false; /* leaves this launch, not finished */
          last_cell = -1;
          last_cell_wide = -1;
        } else if (absorbed) {
          /* PhotonSource::reemit, src/PhotonSource.cpp:272-308 */
          double new_frequency = 0.;
          if (REEMIT)
            new_frequency =
                reemit_decide<FULL, EXACT>(a.model, a.cells, cell_now, rng, p);
          else
            p.type = TYPE_ABSORBED;
          last_cell = -1;
          last_cell_wide = -1;
          done = (new_frequency == 0.);
          if (REEMIT && !done) {
            reemit_launch<FULL, EXACT>(a.grid, a.model, new_frequency, rng, p,
                                       weights);
            if (FULL) {
#pragma unroll
              for (int i = 0; i < CMI_NACC; ++i)
                stage.weight[lane][i] = weights[cmi_acc_of_column(i)];
            }
          }
        }
        if (BUNDLE && done) {
          ended_type = p.type;
          active = false;
        } else if (done) {
          tc0 += (p.type == TYPE_PRIMARY) ? 1u : 0u;
          tc1 += (p.type == TYPE_DIFFUSE_HI) ? 1u : 0u;
          tc2 += (p.type == TYPE_DIFFUSE_HeI) ? 1u : 0u;
          tc3 += (p.type == TYPE_ABSORBED) ? 1u : 0u;
          if (cmi_meta_origin(lane_meta) != 0)
            atomicAdd(&s_continuous[threadIdx.x >> 6][p.type], 1u);
          active = false;
        }
      }
    }
    if (BUNDLE) {
      const unsigned long long ended = wave_ballot(ended_type >= 0);
      const unsigned long long absorbed_lanes =
          wave_ballot(ended_type == TYPE_ABSORBED);
      /* (LDS operations of a wave execute in order: no barrier) */
      if constexpr (POINT) {
        if (lane == 0) {
          unsigned int *all = s_ended[threadIdx.x >> 6];
          all[0] += (unsigned int)__popcll(ended & ~absorbed_lanes);
          all[1] += (unsigned int)__popcll(absorbed_lanes);
        }
      } else if (lane == 0) {
        const unsigned long long continuous_lanes =
            s_continuous_lanes[threadIdx.x >> 6];
        unsigned int *all = s_ended[threadIdx.x >> 6];
        unsigned int *continuous = s_continuous[threadIdx.x >> 6];
        all[0] += (unsigned int)__popcll(ended & ~absorbed_lanes);
        all[1] += (unsigned int)__popcll(absorbed_lanes);
        continuous[TYPE_PRIMARY] +=
            (unsigned int)__popcll(ended & ~absorbed_lanes & continuous_lanes);
        continuous[TYPE_ABSORBED] +=
            (unsigned int)__popcll(absorbed_lanes & continuous_lanes);
      }
    }
    CMI_PHASE_MARK(CMI_PHASE_END);
  }
#ifdef CMI_EXPERIMENTS
  if (stamps && lane == 0) {
    for (int k = 0; k < CMI_PHASE_COUNT; ++k)
      atomicAdd(a.phase_clock + k, phase_cycles[k]);
    /* (the block's waves leave the last flush point together) */
    if (threadIdx.x == 0)
      a.phase_clock[CMI_PHASE_COUNT + 1 + blockIdx.x] =
          __builtin_amdgcn_s_memrealtime();
  }
#endif
#undef CMI_PHASE_MARK
  /* IonizationPhotonShootJobMarket::update_counters */
  /* (BUNDLE: [TYPE_PRIMARY] = ended and not absorbed, [TYPE_ABSORBED]) */
  static_assert(TYPE_PRIMARY == 0 && TYPE_ABSORBED == 3, "the type counts");
  double s0 = BUNDLE ? (double)s_ended[threadIdx.x >> 6][0]
                     : wave_sum((double)tc0);
  double s1 = BUNDLE ? 0. : wave_sum((double)tc1);
  double s2 = BUNDLE ? 0. : wave_sum((double)tc2);
  double s3 = BUNDLE ? (double)s_ended[threadIdx.x >> 6][1]
                     : wave_sum((double)tc3);
  if constexpr (POINT) {
    /* every packet carries the one source's weight */
    const __attribute__((address_space(4))) PointEmitDev *pe =
        (const __attribute__((address_space(4))) PointEmitDev *)point;
    asm volatile("" : "+s"(pe));
    const double w = pe->weight;
    s0 = s0 * w;
    s3 = s3 * w;
  } else {
    /* n packets of a type, c of them from the continuous source:
     * (n - c) w_discrete + c w_continuous */
    const unsigned int *c =
        s_continuous[threadIdx.x >> 6];
    const double w0 = a.model.photon_weight[0], w1 = a.model.photon_weight[1];
    s0 = (s0 - c[0]) * w0 + c[0] * w1;
    s1 = (s1 - c[1]) * w0 + c[1] * w1;
    s2 = (s2 - c[2]) * w0 + c[2] * w1;
    s3 = (s3 - c[3]) * w0 + c[3] * w1;
  }
  double ns = wave_sum((double)nsteps);
  double na = wave_sum((double)natomics);
  if (lane == 0) {
    atomic_add_f64(&counter_shard(a.counters)->totweight, (s0 + s1) + (s2 + s3));
    atomic_add_f64(&counter_shard(a.counters)->typecount[0], s0);
    atomic_add_f64(&counter_shard(a.counters)->typecount[1], s1);
    atomic_add_f64(&counter_shard(a.counters)->typecount[2], s2);
    atomic_add_f64(&counter_shard(a.counters)->typecount[3], s3);
    atomicAdd(&counter_shard(a.counters)->nsteps,
              (unsigned long long)ns + nsteps_wave);
    atomicAdd(&counter_shard(a.counters)->natomics, (unsigned long long)na);
    atomicAdd(&counter_shard(a.counters)->nwavesteps, (unsigned long long)nwavesteps);
  }
