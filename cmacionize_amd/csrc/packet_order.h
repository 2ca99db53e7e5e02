/*
 * packet_order.h - the bucket order: a launch's packets by sort key without
 * a radix sort (included from kernels.h; the host side is order_packets in
 * transport_driver.h, the arithmetic of the plan packet_order_plan.h).
 *
 * Why: the hydrogen-only key is uniformly distributed - the Morton code of
 * two uniform draws, the class from a third -, so a most-significant-digit
 * bucket sort needs neither a histogram pass nor a pass over data it has
 * already placed. The radix sort moves 5.2 GB per 1e8 packets behind the key
 * kernel, this 2.8 GB.
 *
 * How: [bits1 | bits2 | rem_bits] are the key's bits from the top.
 *   1. bucket_key_kernel computes the keys (direction_key_of) and scatters
 *      (key, id) into 2^bits1 regions of fixed capacity;
 *   2. bucket_split_kernel scatters every region into its 2^bits2 leaves,
 *      (the key's last rem_bits, id);
 *   3. bucket_offsets_kernel scans the leaves' counts: their places in the
 *      order;
 *   4. bucket_leaf_kernel orders each leaf in LDS by (remaining bits, id) and
 *      writes its ids. Ties by id: the order does not depend on who was
 *      granted which atomic, and equals the stable radix sort's.
 * A pair that finds its region or leaf full goes to the overflow list, which
 * grows from the back of the order: the order stays a permutation of the
 * launch's ids, whatever the keys' distribution - its tail is then unordered.
 * Every store is guarded by its buffer's capacity; no workgroup waits for
 * another of its launch.
 */
#ifndef CMI_PACKET_ORDER_H
#define CMI_PACKET_ORDER_H

#include "packet_order_plan.h"

#ifndef CMI_BUCKET_THREADS
#define CMI_BUCKET_THREADS 512
#endif
#ifndef CMI_BUCKET_PER_THREAD
#define CMI_BUCKET_PER_THREAD 8
#endif
#define CMI_BUCKET_TILE (CMI_BUCKET_THREADS * CMI_BUCKET_PER_THREAD)
#define CMI_BUCKET_MAX (1 << CMI_BUCKET_LEVEL_BITS)
/* a region's cursor has a 128-B line of its own: every tile of the key
 * kernel adds to every one of them */
#define CMI_BUCKET_REGION_CURSOR_STRIDE 32
#define CMI_BUCKET_LEAF_THREADS 256
#define CMI_BUCKET_LEAF_PER_THREAD                                             \
  (CMI_BUCKET_LEAF_PAIRS / CMI_BUCKET_LEAF_THREADS)
#define CMI_BUCKET_SCAN_THREADS 1024

struct BucketArgs {
  uint32_t n; /* packets of the launch */
  uint32_t key_bits, bits1, bits2, rem_bits;
  uint32_t region_cap, leaf_cap; /* pairs */
  uint2 *regions;                /* [2^bits1][region_cap] */
  uint2 *leaves;                 /* [2^(bits1 + bits2)][leaf_cap] */
  uint32_t *order;               /* [n] */
  /* pairs sent to each region and leaf (those beyond its capacity went to
   * the overflow list), and to the overflow list */
  uint32_t *region_cursor, *leaf_cursor, *overflow_cursor;
  uint32_t *leaf_offset; /* [2^(bits1 + bits2)]: a leaf's place in the order */
  uint32_t *ordered;     /* the ids ahead of the overflow list */
};

struct BucketTileShared {
  uint32_t count[CMI_BUCKET_MAX], start[CMI_BUCKET_MAX], base[CMI_BUCKET_MAX],
      room[CMI_BUCKET_MAX], overflow_at[CMI_BUCKET_MAX];
  uint2 stage[CMI_BUCKET_TILE];
};

/* exclusive prefix sums of count[0, nb), nb <= 256, by the first wave */
__device__ __forceinline__ void bucket_scan_256(const uint32_t *count,
                                                uint32_t *start, uint32_t nb) {
  if (threadIdx.x < 64) {
    uint32_t c[4], total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t bkt = 4u * threadIdx.x + q;
      c[q] = bkt < nb ? count[bkt] : 0u;
      total += c[q];
    }
    uint32_t incl = total;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t below = __shfl_up(incl, off, 64);
      if ((int)threadIdx.x >= off)
        incl += below;
    }
    uint32_t at = incl - total;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t bkt = 4u * threadIdx.x + q;
      if (bkt < nb)
        start[bkt] = at;
      at += c[q];
    }
  }
}

/* A workgroup's m <= CMI_BUCKET_TILE pairs into the nb = 2^bits buckets of
 * digit (key >> shift) & (nb - 1): pair k * CMI_BUCKET_THREADS + threadIdx.x
 * is (key[k], id[k]). Bucket d holds `cap` pairs at dest + d * cap, and
 * cursor[d] counts what was sent to it; the tile's share of a bucket is one
 * run of consecutive places, reserved with one atomic, written from LDS.
 * The stored key is key & keep. What finds its bucket full: a.order, from
 * the back. Called by all threads of the workgroup. */
__device__ __forceinline__ void
bucket_scatter_tile(BucketTileShared &s,
                    const uint32_t (&key)[CMI_BUCKET_PER_THREAD],
                    const uint32_t (&id)[CMI_BUCKET_PER_THREAD], uint32_t m,
                    uint32_t shift, uint32_t nb, uint32_t keep,
                    uint32_t *cursor, uint32_t cursor_stride, uint32_t cap,
                    uint2 *dest, const BucketArgs &a) {
  const uint32_t mask = nb - 1u;
  for (uint32_t d = threadIdx.x; d < nb; d += CMI_BUCKET_THREADS)
    s.count[d] = 0;
  __syncthreads();
  uint32_t rank[CMI_BUCKET_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CMI_BUCKET_PER_THREAD; ++k) {
    rank[k] = 0;
    if ((uint32_t)k * CMI_BUCKET_THREADS + threadIdx.x < m)
      rank[k] = atomicAdd(&s.count[(key[k] >> shift) & mask], 1u);
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < nb; d += CMI_BUCKET_THREADS) {
    const uint32_t cnt = s.count[d];
    const uint32_t base =
        cnt != 0 ? atomicAdd(&cursor[d * cursor_stride], cnt) : 0u;
    const uint32_t left = base < cap ? cap - base : 0u;
    const uint32_t room = cnt < left ? cnt : left;
    s.base[d] = base;
    s.room[d] = room;
    s.overflow_at[d] =
        cnt != room ? atomicAdd(a.overflow_cursor, cnt - room) : 0u;
  }
  bucket_scan_256(s.count, s.start, nb);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CMI_BUCKET_PER_THREAD; ++k)
    if ((uint32_t)k * CMI_BUCKET_THREADS + threadIdx.x < m) {
      /* (< m: the ranks of a bucket are below its count) */
      const uint32_t pos = s.start[(key[k] >> shift) & mask] + rank[k];
      if (pos < CMI_BUCKET_TILE)
        s.stage[pos] = make_uint2(key[k], id[k]);
    }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < m; j += CMI_BUCKET_THREADS) {
    const uint2 pair = s.stage[j];
    const uint32_t d = (pair.x >> shift) & mask;
    const uint32_t r = j - s.start[d];
    if (r < s.room[d]) {
      const uint32_t slot = s.base[d] + r;
      if (slot < cap)
        dest[(uint64_t)d * cap + slot] = make_uint2(pair.x & keep, pair.y);
    } else {
      const uint32_t o = s.overflow_at[d] + (r - s.room[d]);
      if (o < a.n)
        a.order[a.n - 1u - o] = pair.y;
    }
  }
  /* (the barriers of a next call stand between these reads and its writes
   * to everything but the staging array) */
}

/* level 1: the keys of direction_key_kernel, scattered by their top bits1
 * bits. The keys are computed one at a time (the draws are long code) and
 * wait in the thread's own places of the staging array. */
__global__ void __launch_bounds__(CMI_BUCKET_THREADS)
    bucket_key_kernel(const KeyArgs a, const BucketArgs b) {
  __shared__ BucketTileShared s;
  const PacketOrigin from(a.model);
  const uint32_t ntiles = (b.n + CMI_BUCKET_TILE - 1u) / CMI_BUCKET_TILE;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t first = tile * CMI_BUCKET_TILE;
    const uint32_t m =
        b.n - first < CMI_BUCKET_TILE ? b.n - first : CMI_BUCKET_TILE;
#pragma unroll 1
    for (uint32_t local = threadIdx.x; local < m;
         local += CMI_BUCKET_THREADS) {
      uint32_t id;
      const uint32_t key = direction_key_of(a, from, (uint64_t)first + local, id);
      s.stage[local] = make_uint2(key, id);
    }
    uint32_t key[CMI_BUCKET_PER_THREAD], id[CMI_BUCKET_PER_THREAD];
#pragma unroll
    for (int k = 0; k < CMI_BUCKET_PER_THREAD; ++k) {
      const uint32_t local = (uint32_t)k * CMI_BUCKET_THREADS + threadIdx.x;
      const uint2 pair = local < m ? s.stage[local] : make_uint2(0u, 0u);
      key[k] = pair.x;
      id[k] = pair.y;
    }
    bucket_scatter_tile(s, key, id, m, b.key_bits - b.bits1, 1u << b.bits1,
                        0xffffffffu, b.region_cursor,
                        CMI_BUCKET_REGION_CURSOR_STRIDE, b.region_cap,
                        b.regions, b);
    __syncthreads(); /* the staging array is rewritten by the next tile */
  }
}

/* level 2: tile blockIdx.x of region blockIdx.y into the region's leaves */
__global__ void __launch_bounds__(CMI_BUCKET_THREADS)
    bucket_split_kernel(const BucketArgs b) {
  __shared__ BucketTileShared s;
  const uint32_t region = blockIdx.y;
  const uint32_t sent =
      b.region_cursor[region * CMI_BUCKET_REGION_CURSOR_STRIDE];
  const uint32_t held = sent < b.region_cap ? sent : b.region_cap;
  const uint64_t first = (uint64_t)blockIdx.x * CMI_BUCKET_TILE;
  if (first >= held)
    return;
  const uint32_t m = held - first < CMI_BUCKET_TILE ? (uint32_t)(held - first)
                                                    : CMI_BUCKET_TILE;
  const uint2 *from = b.regions + (uint64_t)region * b.region_cap + first;
  uint32_t key[CMI_BUCKET_PER_THREAD], id[CMI_BUCKET_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CMI_BUCKET_PER_THREAD; ++k) {
    const uint32_t local = (uint32_t)k * CMI_BUCKET_THREADS + threadIdx.x;
    const uint2 pair = local < m ? from[local] : make_uint2(0u, 0u);
    key[k] = pair.x;
    id[k] = pair.y;
  }
  const uint64_t leaf0 = (uint64_t)region << b.bits2;
  bucket_scatter_tile(s, key, id, m, b.rem_bits, 1u << b.bits2,
                      (1u << b.rem_bits) - 1u, b.leaf_cursor + leaf0, 1u,
                      b.leaf_cap, b.leaves + leaf0 * b.leaf_cap, b);
}

/* the leaves' places in the order: exclusive prefix sums of the pairs they
 * hold. Workgroup c takes the leaves [c, c + 1) * CMI_BUCKET_SCAN_THREADS: it
 * adds up the leaves ahead of them itself (at most 256 KB, from the L2) - no
 * workgroup waits for another - and scans its own. */
__device__ __forceinline__ uint32_t bucket_leaf_held(const BucketArgs &b,
                                                     uint32_t leaf,
                                                     uint32_t nleaves) {
  if (leaf >= nleaves)
    return 0u;
  const uint32_t sent = b.leaf_cursor[leaf];
  return sent < b.leaf_cap ? sent : b.leaf_cap;
}

__global__ void __launch_bounds__(CMI_BUCKET_SCAN_THREADS)
    bucket_offsets_kernel(const BucketArgs b) {
  constexpr uint32_t WAVES = CMI_BUCKET_SCAN_THREADS / 64;
  __shared__ uint32_t wave_ahead[WAVES], wave_total[WAVES];
  const uint32_t nleaves = 1u << (b.bits1 + b.bits2);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t ahead = 0;
#pragma unroll 8
  for (uint32_t c = 0; c < blockIdx.x; ++c)
    ahead += bucket_leaf_held(b, c * CMI_BUCKET_SCAN_THREADS + threadIdx.x,
                              nleaves);
  const uint32_t leaf = blockIdx.x * CMI_BUCKET_SCAN_THREADS + threadIdx.x;
  const uint32_t mine = bucket_leaf_held(b, leaf, nleaves);
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t below = __shfl_up(incl, off, 64);
    const uint32_t more = __shfl_xor(ahead, off, 64);
    if ((int)lane >= off)
      incl += below;
    ahead += more; /* (a butterfly: every lane ends with the wave's sum) */
  }
  if (lane == 63) {
    wave_total[wave] = incl;
    wave_ahead[wave] = ahead;
  }
  __syncthreads();
  uint32_t at = incl - mine, all = 0;
  for (uint32_t w = 0; w < WAVES; ++w) {
    at += wave_ahead[w];
    if (w < wave)
      at += wave_total[w];
    all += wave_ahead[w] + wave_total[w];
  }
  if (leaf < nleaves)
    b.leaf_offset[leaf] = at;
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1)
    *b.ordered = all;
}

/* a leaf's pairs by (remaining key bits, id): binned by the bits in LDS, the
 * ids of a bin ranked against each other, the ids written in runs. The
 * pairs are loaded before their count is known (whatever of the leaf's room
 * was not written is not looked at). */
__global__ void __launch_bounds__(CMI_BUCKET_LEAF_THREADS)
    bucket_leaf_kernel(const BucketArgs b) {
  __shared__ uint32_t s_count[CMI_BUCKET_MAX], s_start[CMI_BUCKET_MAX];
  __shared__ uint32_t s_binned[CMI_BUCKET_LEAF_PAIRS];
  __shared__ uint32_t s_sorted[CMI_BUCKET_LEAF_PAIRS];
  const uint32_t leaf = blockIdx.x;
  const uint32_t room =
      b.leaf_cap < CMI_BUCKET_LEAF_PAIRS ? b.leaf_cap : CMI_BUCKET_LEAF_PAIRS;
  const uint2 *from = b.leaves + (uint64_t)leaf * b.leaf_cap;
  uint2 pair[CMI_BUCKET_LEAF_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CMI_BUCKET_LEAF_PER_THREAD; ++k) {
    const uint32_t j = (uint32_t)k * CMI_BUCKET_LEAF_THREADS + threadIdx.x;
    pair[k] = j < room ? from[j] : make_uint2(0u, 0u);
  }
  const uint32_t sent = b.leaf_cursor[leaf];
  const uint32_t held = sent < room ? sent : room;
  if (held == 0)
    return;
  const uint32_t offset = b.leaf_offset[leaf];
  const uint32_t nb = 1u << b.rem_bits, mask = nb - 1u;
  for (uint32_t d = threadIdx.x; d < nb; d += CMI_BUCKET_LEAF_THREADS)
    s_count[d] = 0;
  __syncthreads();
  uint32_t rank[CMI_BUCKET_LEAF_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CMI_BUCKET_LEAF_PER_THREAD; ++k) {
    const uint32_t j = (uint32_t)k * CMI_BUCKET_LEAF_THREADS + threadIdx.x;
    pair[k].x &= mask;
    rank[k] = j < held ? atomicAdd(&s_count[pair[k].x], 1u) : 0u;
  }
  __syncthreads();
  bucket_scan_256(s_count, s_start, nb);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CMI_BUCKET_LEAF_PER_THREAD; ++k) {
    const uint32_t j = (uint32_t)k * CMI_BUCKET_LEAF_THREADS + threadIdx.x;
    if (j < held) {
      const uint32_t pos = s_start[pair[k].x] + rank[k];
      if (pos < CMI_BUCKET_LEAF_PAIRS)
        s_binned[pos] = pair[k].y;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CMI_BUCKET_LEAF_PER_THREAD; ++k) {
    const uint32_t j = (uint32_t)k * CMI_BUCKET_LEAF_THREADS + threadIdx.x;
    if (j < held) {
      const uint32_t begin = s_start[pair[k].x];
      const uint32_t end = begin + s_count[pair[k].x];
      uint32_t smaller = 0;
      for (uint32_t i = begin; i < end && i < CMI_BUCKET_LEAF_PAIRS; ++i)
        smaller += s_binned[i] < pair[k].y ? 1u : 0u;
      if (begin + smaller < CMI_BUCKET_LEAF_PAIRS)
        s_sorted[begin + smaller] = pair[k].y;
    }
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < held; j += CMI_BUCKET_LEAF_THREADS)
    if ((uint64_t)offset + j < b.n)
      b.order[offset + j] = s_sorted[j];
}

/* the keys of the packets in a launch's order, for the host to look at
 * (cmi_gpu_order_packets); an id that is no packet of the launch: all ones */
__global__ void order_probe_kernel(const KeyArgs a, const uint32_t *order,
                                   uint32_t *keys) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const PacketOrigin from(a.model);
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       j < a.n_packets; j += stride) {
    const uint32_t id = order[j];
    uint32_t unused;
    keys[j] = id < a.n_packets ? direction_key_of(a, from, id, unused)
                               : 0xffffffffu;
  }
}

#endif /* CMI_PACKET_ORDER_H */
