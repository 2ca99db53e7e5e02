/*
 * packet_order_plan.h - the host arithmetic of the bucket order
 * (packet_order.h): how many bits each scatter level takes, how many pairs a
 * region and a leaf hold, and where they lie in the sort buffers. Plain C++
 * with no device code, so that a stand-alone program can call it
 * (tests/test_packet_order_plan.py).
 */
#ifndef CMI_PACKET_ORDER_PLAN_H
#define CMI_PACKET_ORDER_PLAN_H

#include <cmath>
#include <cstdint>

/* most bits of one scatter level (its counters live in LDS) */
#define CMI_BUCKET_LEVEL_BITS 8
/* most key bits left for the leaf kernel to order */
#define CMI_BUCKET_REM_BITS 8
/* most pairs of a leaf: 8 B each in LDS and 4 B for the ordered ids, 30 KB
 * (a mean leaf of 2047 pairs and its 9 deviations are 2463) */
#define CMI_BUCKET_LEAF_PAIRS 2560
/* most pairs of one leaf that may share their remaining key bits on average
 * (the leaf kernel ranks those by id against each other) */
#define CMI_BUCKET_TIE_PAIRS 256
/* the Poisson spread the default capacities leave room for */
#define CMI_BUCKET_SIGMAS_REGION 12.
#define CMI_BUCKET_SIGMAS_LEAF 9.

struct BucketPlan {
  int take;          /* 0: the radix sort orders this launch */
  int bits1, bits2;  /* bits of the two scatter levels */
  int rem_bits;      /* key bits left for the leaves */
  uint32_t region_cap, leaf_cap; /* pairs */
  /* 32-bit words from the start of the sort buffers: the order lies at
   * [0, n) - the leaves' ids from the front, the overflow list from the
   * back -, the regions at [region_begin, region_begin + region_words), the
   * leaves at [leaf_begin, total_words) */
  uint64_t region_begin, region_words, leaf_begin, total_words;
};

/* pairs a bucket of `mean` expected pairs holds: the mean and `sigmas` Poisson
 * deviations, or - slack_permille >= 0 - the mean and that many thousandths
 * of it */
static inline uint64_t cmi_bucket_capacity(double mean, double sigmas,
                                           int slack_permille) {
  const double cap = slack_permille >= 0
                         ? mean * (1000. + (double)slack_permille) / 1000.
                         : mean + sigmas * std::sqrt(mean) + 8.;
  const uint64_t c = (uint64_t)std::ceil(cap);
  return c < 1 ? 1 : c;
}

/* The plan for a launch of n packets with keys of key_bits bits. bits1, bits2
 * and slack_permille < 0: chosen here - as many bits as leave a mean leaf
 * 1024 to 2047 pairs, the upper half of them for the first level. */
static inline BucketPlan cmi_bucket_plan(uint64_t n, int key_bits, int bits1,
                                         int bits2, int slack_permille,
                                         uint64_t min_packets) {
  BucketPlan b = {};
  if (n == 0 || n < min_packets || n >= ((uint64_t)1 << 31) || key_bits < 0 ||
      key_bits > 32)
    return b;
  int total = 0;
  while (total < 2 * CMI_BUCKET_LEVEL_BITS && (n >> (total + 1)) >= 1024)
    ++total;
  if (total > key_bits)
    total = key_bits;
  b.bits1 = bits1 >= 0 ? bits1 : (total + 1) / 2;
  b.bits2 = bits2 >= 0 ? bits2 : total - (total + 1) / 2;
  if (b.bits1 > CMI_BUCKET_LEVEL_BITS || b.bits2 > CMI_BUCKET_LEVEL_BITS)
    return b;
  b.rem_bits = key_bits - b.bits1 - b.bits2;
  if (b.rem_bits < 0 || b.rem_bits > CMI_BUCKET_REM_BITS)
    return b;
  const double mean1 = (double)n / (double)((uint64_t)1 << b.bits1);
  const double mean2 = mean1 / (double)((uint64_t)1 << b.bits2);
  if (mean2 / (double)(1u << b.rem_bits) > (double)CMI_BUCKET_TIE_PAIRS)
    return b;
  const uint64_t cap1 =
      cmi_bucket_capacity(mean1, CMI_BUCKET_SIGMAS_REGION, slack_permille);
  const uint64_t cap2 =
      cmi_bucket_capacity(mean2, CMI_BUCKET_SIGMAS_LEAF, slack_permille);
  if (cap2 > CMI_BUCKET_LEAF_PAIRS || cap1 >= ((uint64_t)1 << 31))
    return b;
  b.region_cap = (uint32_t)cap1;
  b.leaf_cap = (uint32_t)cap2;
  b.region_words = 2 * (cap1 << b.bits1);
  b.region_begin = (n + 63) & ~(uint64_t)63;
  b.leaf_begin = (b.region_begin + b.region_words + 63) & ~(uint64_t)63;
  b.total_words = b.leaf_begin + 2 * (cap2 << (b.bits1 + b.bits2));
  b.take = 1;
  return b;
}

#endif /* CMI_PACKET_ORDER_PLAN_H */
