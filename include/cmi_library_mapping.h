/*
 * cmi_library_mapping.h - the device mapping of libcmi_gpu_library.so: the
 * switch that makes the library mode of include/cmi_library.h map SPH
 * particles onto cells and back with the device operators of
 * include/cmi_gpu.h ("SPH mappings"), and the two mapping probes of
 * cmi_library.h through those operators. Not in the reference.
 */
#ifndef CMI_LIBRARY_MAPPING_H
#define CMI_LIBRARY_MAPPING_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Device mapping: with a non-zero value cmi_compute_neutral_fraction_* maps
 * the particles onto the cells and the cells back onto the particles with
 * the device operators of include/cmi_gpu.h ("SPH mappings") - mapping type
 * "centroid" only, and only when the call does not decline (then, and for
 * every other mapping type, the host path runs; with talk on the library says
 * which path ran and why). 0: the host path. Until the first call the
 * environment decides: CMI_GPU_DEVICE_MAPPING=1 switches it on, anything
 * else - the default - leaves the host path. The two probes of cmi_library.h
 * stay on the host whatever the switch says. */
void cmi_gpu_library_set_device_mapping(int on);
/* how many calls of the two device operators this library has made and not
 * seen declined, since it was loaded */
long cmi_gpu_library_device_mapping_count();

/* The two probes through the device operators ("centroid" only), on the
 * device CMI_GPU_DEVICE names, whatever the switch says. Return 0, 2 when
 * the call declined (why on stderr, nothing written), or 1 with a message on
 * stderr. */
int cmi_gpu_library_device_map_to_cells(
    const char *mapping_type, int precision, const void *x, const void *y,
    const void *z, const void *h, const void *m, size_t N,
    double unit_length_in_SI, double unit_mass_in_SI,
    const double *periodic_box, const double *grid_anchor,
    const double *grid_sides, const int *ncell, double *number_density);
int cmi_gpu_library_device_map_to_particles(
    const char *mapping_type, int precision, const void *x, const void *y,
    const void *z, const void *h, const void *m, size_t N,
    double unit_length_in_SI, double unit_mass_in_SI,
    const double *periodic_box, const double *grid_anchor,
    const double *grid_sides, const int *ncell,
    const double *neutral_fraction_of_cells, double *nH);

#ifdef __cplusplus
}
#endif

#endif
