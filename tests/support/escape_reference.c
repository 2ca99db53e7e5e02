/*
 * escape_reference.c - test infrastructure: the CPU restatement of the escape
 * tally (include/cmi_gpu.h, "escape maps").
 *
 * cmio_shoot's packet loop (oracle/cmio_transport.c, restating
 * src/IonizationPhotonShootJob.hpp:117-146) with the tally at its end: a
 * packet whose last flight left the box adds its weight to
 * sky[(type nfreq + bin) nlon nmu + i nmu + j]. The loop needs the oracle's
 * file-static random_photon and reemit, so that file is part of this
 * translation unit; the rest of the oracle comes from libcmio.so. The binning
 * formulae are written out here, from the contract, not taken from the
 * engine's device header.
 *
 * Besides the tally the call reports how close any escaped packet came to an
 * edge: the bit-for-bit comparison with the engine excuses no packet, which
 * is safe only while no packet sits within the last bits (the device's atan2,
 * sincos and log differ from the host's there) of a pixel or bin edge.
 */
#include "../../oracle/cmio_transport.c"

/* src/LevelFrequencyBins.hpp:52-66: the ionization energies of
 * src/ElementData.hpp:39-105 in Hz, ascending, closed by four times
 * hydrogen's */
static const double escref_level_edges[CMIO_NION + 1] = {
    3.28810279e+15, 3.29284691e+15, 3.51435505e+15, 5.21432028e+15,
    5.64310422e+15, 5.89588678e+15, 5.94523574e+15, 7.15759434e+15,
    8.41222200e+15, 8.49136314e+15, 9.90492110e+15, 1.14182796e+16,
    1.14732262e+16, 1.15792700e+16, 4. * 3.28810279e+15};

/* interior edge k (1 <= k < nfreq) of the bins: what lies below the first
 * edge or above the last is clamped into the end bins, so those two are no
 * edges of the binning */
static double escref_bin_edge(int32_t bins_type, int32_t nfreq, double minimum,
                              double maximum, int32_t k) {
  if (bins_type == 1)
    return escref_level_edges[k];
  return minimum + (maximum - minimum) * k / nfreq;
}

static int32_t escref_bin(int32_t bins_type, int32_t nfreq, double minimum,
                          double maximum, double frequency) {
  if (bins_type == 1) {
    /* the last edge below the frequency, the end bins for what lies outside */
    int32_t bin = 0;
    for (int32_t k = 1; k < CMIO_NION; ++k)
      if (frequency > escref_level_edges[k])
        bin = k;
    return bin;
  }
  if (frequency < minimum)
    return 0;
  if (frequency >= maximum)
    return nfreq - 1;
  return (int32_t)((frequency - minimum) * (nfreq / (maximum - minimum)));
}

/* frame[9]: e_1, e_2, e_3 as rows. sky[3 nfreq nlon nmu] is added to.
 * edge_distance[0]: the smallest |l - edge| (radians, the seam at +-pi is an
 * edge) and |mu - edge| (interior edges) over all escaped packets;
 * edge_distance[1]: the smallest |nu - edge| / edge over the interior bin
 * edges. Both start at what the caller put there. */
void escref_shoot(const cmio_grid *grid, const cmio_model *model,
                  cmio_cells *cells, uint32_t seed, uint32_t iteration,
                  uint64_t first_packet, uint64_t n_packets, double *totweight,
                  double typecount[CMIO_NTYPE], const double *frame,
                  int32_t nlon, int32_t nmu, int32_t nfreq, int32_t bins_type,
                  double minimum_frequency, double maximum_frequency,
                  double *sky, double *edge_distance) {
  double tw = 0.;
  double tc0 = 0., tc1 = 0., tc2 = 0., tc3 = 0.;
  double near_pixel = edge_distance[0], near_bin = edge_distance[1];
#pragma omp parallel for schedule(dynamic, 1024)                              \
    reduction(+ : tw, tc0, tc1, tc2, tc3) reduction(min : near_pixel, near_bin)
  for (uint64_t i = 0; i < n_packets; ++i) {
    cmio_rng rng = {seed, iteration, first_packet + i, 0, NULL};
    cmio_photon photon;
    random_photon(model, &rng, &photon);
    double tau = -log(cmio_rng_next(&rng));
    int64_t cell =
        cmio_interact(grid, model, cells, &photon, tau, NULL, NULL, 0, NULL);
    while (cell >= 0 && reemit(model, cells, cell, &photon, &rng)) {
      tau = -log(cmio_rng_next(&rng));
      cell =
          cmio_interact(grid, model, cells, &photon, tau, NULL, NULL, 0, NULL);
    }
    tw += photon.weight;
    switch (photon.type) {
    case CMIO_TYPE_PRIMARY:
      tc0 += photon.weight;
      break;
    case CMIO_TYPE_DIFFUSE_HI:
      tc1 += photon.weight;
      break;
    case CMIO_TYPE_DIFFUSE_HeI:
      tc2 += photon.weight;
      break;
    default:
      tc3 += photon.weight;
      break;
    }
    /* ---- the tally: the packet's flight ended outside the box ---- */
    if (cell >= 0 || photon.type < 0 || photon.type > 2)
      continue;
    const double *d = photon.direction;
    const double x = d[0] * frame[0] + d[1] * frame[1] + d[2] * frame[2];
    const double y = d[0] * frame[3] + d[1] * frame[4] + d[2] * frame[5];
    const double mu = d[0] * frame[6] + d[1] * frame[7] + d[2] * frame[8];
    const double l = atan2(y, x);
    const double fj = (mu + 1.) / 2. * nmu;
    const double fi = (l + M_PI) / (2. * M_PI) * nlon;
    int32_t j = (int32_t)floor(fj), ii = (int32_t)floor(fi);
    if (j > nmu - 1)
      j = nmu - 1;
    if (j < 0)
      j = 0;
    if (ii > nlon - 1)
      ii = nlon - 1;
    if (ii < 0)
      ii = 0;
    const int32_t bin = escref_bin(bins_type, nfreq, minimum_frequency,
                                   maximum_frequency, photon.energy);
    double *at = sky +
                 ((size_t)photon.type * (size_t)nfreq + (size_t)bin) *
                     ((size_t)nlon * (size_t)nmu) +
                 (size_t)ii * (size_t)nmu + (size_t)j;
#pragma omp atomic
    *at += photon.weight;
    /* distances to the edges */
    for (int32_t k = 0; k <= nlon; ++k) {
      const double edge = -M_PI + 2. * M_PI * k / nlon;
      if (fabs(l - edge) < near_pixel)
        near_pixel = fabs(l - edge);
    }
    for (int32_t k = 1; k < nmu; ++k) {
      const double edge = -1. + 2. * k / nmu;
      if (fabs(mu - edge) < near_pixel)
        near_pixel = fabs(mu - edge);
    }
    for (int32_t k = 1; k < nfreq; ++k) {
      const double edge = escref_bin_edge(bins_type, nfreq, minimum_frequency,
                                          maximum_frequency, k);
      if (fabs(photon.energy - edge) / edge < near_bin)
        near_bin = fabs(photon.energy - edge) / edge;
    }
  }
  *totweight += tw;
  typecount[0] += tc0;
  typecount[1] += tc1;
  typecount[2] += tc2;
  typecount[3] += tc3;
  edge_distance[0] = near_pixel;
  edge_distance[1] = near_bin;
}

/* the pixel i nmu + j of n unit vectors by the formulae above */
void escref_pixels(const double *frame, int32_t nlon, int32_t nmu, int64_t n,
                   const double *directions, int32_t *pixels) {
  for (int64_t k = 0; k < n; ++k) {
    const double *d = directions + 3 * k;
    const double x = d[0] * frame[0] + d[1] * frame[1] + d[2] * frame[2];
    const double y = d[0] * frame[3] + d[1] * frame[4] + d[2] * frame[5];
    const double mu = d[0] * frame[6] + d[1] * frame[7] + d[2] * frame[8];
    int32_t j = (int32_t)floor((mu + 1.) / 2. * nmu);
    int32_t i = (int32_t)floor((atan2(y, x) + M_PI) / (2. * M_PI) * nlon);
    j = j < 0 ? 0 : (j > nmu - 1 ? nmu - 1 : j);
    i = i < 0 ? 0 : (i > nlon - 1 ? nlon - 1 : i);
    pixels[k] = i * nmu + j;
  }
}
