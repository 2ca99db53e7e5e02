"""ctypes binding of the engine's C ABI (include/cmi_gpu.h, libcmi_gpu.so).

This is plumbing only: every method is one call through the C ABI. There is no
Python or CPU implementation of the path behind it - if the HIP library is
missing or no device is present, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CMI_GPU_LIBRARY: load another build of the same library (kernel experiments)
LIB_PATH = os.environ.get("CMI_GPU_LIBRARY",
                          os.path.join(_HERE, "libcmi_gpu.so"))

NION = 14
TRACKER_SPECTRUM, TRACKER_ABSORPTION, TRACKER_WEIGHTED_SPECTRUM = 0, 1, 2
NACC = 16
NTYPE = 4

FIELD_NUMBER_DENSITY = 0
FIELD_TEMPERATURE = 1
FIELD_IONIC_FRACTION = 2
FIELD_MEAN_INTENSITY = 16
FIELD_HEATING = 30

REEMIT_NONE, REEMIT_PHYSICAL, REEMIT_FIXED = 0, 1, 2
# how a launch's packets were ordered (GpuEngine.order_plan)
ORDER_NONE, ORDER_RADIX, ORDER_BUCKET = 0, 1, 2
CONTINUOUS_NONE, CONTINUOUS_ISOTROPIC, CONTINUOUS_PLANAR = 0, 1, 2
# cmi_gpu_set_*_table (the generic lowering of a plugin into a table)
ROLE_SOURCE, ROLE_CONTINUOUS = 0, 1
TABLE_LINEAR, TABLE_LOGLOG = 0, 1
# cmi_gpu_dust_probe kinds
DUST_PROBE_EMIT, DUST_PROBE_SCATTER, DUST_PROBE_SCATTER_TOWARDS = 0, 1, 2
DUST_PROBE_OPTICAL_DEPTH, DUST_PROBE_TRACE = 3, 4
DUST_PROBE_CELL_SOURCE = 5
DUST_PROBE_SKY_PEEL = 6
DUST_PROBE_CUBE_TRACE = 7
# cmi_gpu_lya_probe kinds, and the largest cap on a packet's scatterings
LYA_PROBE_VOIGT, LYA_PROBE_OPTICAL_DEPTH = 0, 1
LYA_PROBE_SAMPLER, LYA_PROBE_TRACE = 2, 3
LYA_MAX_SCATTER = 100000000
LYA_LAMBDA0 = 1215.67e-10  # m
# the columns of a row of cmi_gpu_download_lya_field
LYA_FIELD_COLUMNS = ("L", "S_H", "S_d", "G_x", "G_y", "G_z", "N_H", "N_d")
# CMI_GPU_MAX_VIEWS: the views of one run (set_ccd_images, set_sky_cameras)
MAX_VIEWS = 64

_dp = C.POINTER(C.c_double)


class Config(C.Structure):
    _fields_ = [("anchor", C.c_double * 3), ("sides", C.c_double * 3),
                ("ncell", C.c_int32 * 3), ("periodic", C.c_int32 * 3),
                ("device", C.c_int32), ("track_heating", C.c_int32),
                ("stream", C.c_void_p),
                ("external_accumulators", C.c_void_p),
                ("sub_offset", C.c_int32 * 3), ("sub_ncell", C.c_int32 * 3)]


class TemperatureParams(C.Structure):
    _fields_ = [("do_temperature_calculation", C.c_int32),
                ("minimum_number_of_iterations", C.c_int32),
                ("epsilon_convergence", C.c_double),
                ("maximum_number_of_iterations", C.c_int32),
                ("pah_heating_factor", C.c_double),
                ("cosmic_ray_heating_factor", C.c_double),
                ("cosmic_ray_heating_limit", C.c_double),
                ("cosmic_ray_heating_scale_length", C.c_double),
                ("minimum_ionized_temperature", C.c_double)]


class EngineError(RuntimeError):
    pass


class SphMapDeclined(EngineError):
    """An SPH mapping declined (include/cmi_gpu.h, "SPH mappings"): nothing was
    computed and the caller runs the host path. `reason` is one of
    SPH_DECLINE_REASONS."""

    def __init__(self, message, reason):
        EngineError.__init__(self, message)
        self.reason = reason


EDECLINED = 5
SPH_KERNELS = {"spline_h": 0, "spline_2h": 1}
SPH_DECLINE_REASONS = {1: "no_particles", 2: "wide_kernel", 3: "list_size"}


# every symbol include/cmi_gpu.h declares
EXPORTED_SYMBOLS = [
    "cmi_gpu_create", "cmi_gpu_destroy", "cmi_gpu_last_error",
    "cmi_gpu_synchronize", "cmi_gpu_number_of_cells", "cmi_gpu_set_sources",
    "cmi_gpu_set_spectrum_monochromatic", "cmi_gpu_set_spectrum_planck",
    "cmi_gpu_set_continuous_source",
    "cmi_gpu_set_continuous_source_planar",
    "cmi_gpu_set_continuous_spectrum_monochromatic",
    "cmi_gpu_set_continuous_spectrum_planck",
    "cmi_gpu_set_cross_sections_fixed", "cmi_gpu_set_cross_sections_verner",
    "cmi_gpu_set_spectrum_table", "cmi_gpu_set_cross_sections_table",
    "cmi_gpu_set_recombination_rates_table",
    "cmi_gpu_set_recombination_rates_fixed",
    "cmi_gpu_set_recombination_rates_verner", "cmi_gpu_set_abundances",
    "cmi_gpu_set_reemission", "cmi_gpu_set_temperature_params",
    "cmi_gpu_upload_cells", "cmi_gpu_upload_field", "cmi_gpu_download_field",
    "cmi_gpu_field_device_pointer", "cmi_gpu_reset_grid", "cmi_gpu_shoot",
    "cmi_gpu_get_counters", "cmi_gpu_update_cells", "cmi_gpu_emit_packets",
    "cmi_gpu_trace_packets", "cmi_gpu_get_timing", "cmi_gpu_set_tuning",
    "cmi_gpu_get_atomic_count", "cmi_gpu_sample_spectrum",
    "cmi_gpu_thermal_probe", "cmi_gpu_accumulator_layout",
    "cmi_gpu_get_kernel_timing", "cmi_gpu_get_wave_steps",
    "cmi_gpu_get_launch_times", "cmi_gpu_set_export_buffer",
    "cmi_gpu_get_export_count", "cmi_gpu_reset_exports",
    "cmi_gpu_shoot_flights", "cmi_gpu_download_exports",
    "cmi_gpu_shoot_flights_host", "cmi_gpu_physics_probe",
    "cmi_gpu_update_cells_range", "cmi_gpu_refresh_transport_records",
    "cmi_gpu_get_launch_steps", "cmi_gpu_group_create",
    "cmi_gpu_group_destroy", "cmi_gpu_group_reduce_accumulators",
    "cmi_gpu_group_update_cells",
    "cmi_gpu_group_exchange_flights", "cmi_gpu_group_exchange_stats",
    "cmi_gpu_compute_emissivities",
    "cmi_gpu_set_spectrum_trackers", "cmi_gpu_enable_trackers",
    "cmi_gpu_get_tracker_counts", "cmi_gpu_set_trackers",
    "cmi_gpu_get_tracker_absorption", "cmi_gpu_set_tracker_frequency_bins",
    "cmi_gpu_get_tracker_flux", "cmi_gpu_projected_areas",
    "cmi_gpu_set_dust_scattering", "cmi_gpu_set_ccd_image",
    "cmi_gpu_set_continuous_source_spiral_galaxy", "cmi_gpu_dust_shoot",
    "cmi_gpu_download_image", "cmi_gpu_reset_image",
    "cmi_gpu_get_dust_counters", "cmi_gpu_dust_probe",
    "cmi_gpu_render_line_images", "cmi_gpu_render_field_images",
    "cmi_gpu_line_image_probe",
    "cmi_gpu_set_dust_scattering_per_hydrogen",
    "cmi_gpu_set_cell_source_line", "cmi_gpu_set_cell_source_field",
    "cmi_gpu_get_cell_source",
    "cmi_gpu_render_line_sky", "cmi_gpu_render_field_sky",
    "cmi_gpu_sky_probe", "cmi_gpu_render_line_sky_map",
    "cmi_gpu_sky_map_directions",
    "cmi_gpu_set_sky_camera", "cmi_gpu_check_sky_camera",
    "cmi_gpu_get_sky_camera_counters",
    "cmi_gpu_set_ccd_images", "cmi_gpu_set_sky_cameras",
    "cmi_gpu_download_image_view", "cmi_gpu_get_dust_view_counters",
    "cmi_gpu_select_probe_view",
    "cmi_gpu_set_cell_velocities", "cmi_gpu_render_line_cube",
    "cmi_gpu_render_field_cube", "cmi_gpu_emission_line_atomic_weight",
    "cmi_gpu_render_field_sky_cube", "cmi_gpu_render_line_sky_cube",
    "cmi_gpu_render_line_sky_map_cube",
    "cmi_gpu_set_scattered_cube", "cmi_gpu_download_cube_view",
    "cmi_gpu_get_phase_clocks",
    "cmi_gpu_free_free_coefficients", "cmi_gpu_render_continuum_images",
    "cmi_gpu_render_field_continuum_images", "cmi_gpu_render_continuum_sky",
    "cmi_gpu_render_field_continuum_sky",
    "cmi_gpu_render_continuum_sky_map", "cmi_gpu_continuum_probe",
    "cmi_gpu_hi_coefficients", "cmi_gpu_render_hi_cube",
    "cmi_gpu_render_hi_sky_cube", "cmi_gpu_render_hi_sky_map_cube",
    "cmi_gpu_render_field_absorbing_cube",
    "cmi_gpu_render_field_absorbing_sky_cube",
    "cmi_gpu_absorbing_cube_probe", "cmi_gpu_get_update_state",
    "cmi_gpu_set_lyman_alpha", "cmi_gpu_lya_shoot", "cmi_gpu_lya_probe",
    "cmi_gpu_download_lya_view", "cmi_gpu_reset_lya",
    "cmi_gpu_get_lya_counters", "cmi_gpu_lyman_alpha_emissivity",
    "cmi_gpu_set_lya_field", "cmi_gpu_download_lya_field",
    "cmi_gpu_lya_spin_temperature",
    "cmi_gpu_render_field_absorption_spectra",
    "cmi_gpu_render_absorption_spectra", "cmi_gpu_absorption_probe",
    "cmi_gpu_set_escape_tally", "cmi_gpu_reset_escape_tally",
    "cmi_gpu_download_escape_tally", "cmi_gpu_escape_pixels",
    "cmi_gpu_cross_sections", "cmi_gpu_get_transport_plan",
    "cmi_gpu_get_order_plan", "cmi_gpu_order_packets",
    "cmi_gpu_get_bundle_march", "cmi_gpu_get_bundle_point",
    "cmi_gpu_sph_map_to_cells", "cmi_gpu_sph_map_to_particles",
    "cmi_gpu_get_sph_map_stats",
]

# the emission lines of EmissivityValues (src/EmissivityValues.hpp:36-81), in
# the order cmi_gpu_compute_emissivities numbers them
EMISSION_LINES = [
    "HAlpha", "HBeta", "HII", "BALMER_JUMP_LOW", "BALMER_JUMP_HIGH",
    "OI_6300", "OI_6364", "OII_3727", "OIII_5007", "OIII_4959", "OIII_4363",
    "OIII_52mu", "OIII_88mu", "NII_5755", "NII_6548", "NII_6584",
    "NeIII_3869", "NeIII_3968", "SII_6725", "SII_4072", "SIII_9405",
    "SIII_6312", "SIII_19mu", "SIII_33mu", "avg_T", "avg_T_count",
    "avg_nH_nHe", "avg_nH_nHe_count", "NeII_12mu", "NIII_57mu", "NeIII_15mu",
    "NII_122mu", "CII_158mu", "CII_2325", "CIII_1908", "OII_7325", "SIV_10mu",
    "HeI_5876", "Hrec_s", "WFC2_F439W", "WFC2_F555W", "WFC2_F675W"]

# standard atomic weights of the emitting elements: the entries of
# EMISSION_LINES that are the line of one ion, hence have a spectral cube
_ELEMENT_WEIGHTS = {"H": 1.00794, "He": 4.002602, "C": 12.0107, "N": 14.0067,
                    "O": 15.9994, "Ne": 20.1797, "S": 32.065}


def _line_element(name):
    if name in ("HAlpha", "HBeta"):
        return "H"
    for element in ("He", "Ne", "C", "N", "O", "S"):
        if name.startswith(element + "I"):
            return element
    return None


LINE_ATOMIC_WEIGHTS = {name: _ELEMENT_WEIGHTS[_line_element(name)]
                       for name in EMISSION_LINES
                       if name != "HII" and _line_element(name)}


def cube_channel_centres(nchan, vmin, vmax):
    """Centres (m s^-1) of the channels of a cube over [vmin, vmax): the
    means of the edges vmin + c * dv."""
    dv = (vmax - vmin) / nchan
    edges = vmin + np.arange(nchan + 1) * dv
    return 0.5 * (edges[:-1] + edges[1:])


def cube_moments(cube, centres):
    """Moments of a cube (..., nchan, nx, ny) along its channel axis: moment
    0 (the sum over channels), the intensity-weighted mean velocity and the
    dispersion about it, each (..., nx, ny); the last two are NaN where
    moment 0 is 0."""
    cube = np.asarray(cube, dtype=np.float64)
    v = np.asarray(centres, dtype=np.float64)[:, None, None]
    m0 = cube.sum(axis=-3)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(m0 == 0., np.nan, (cube * v).sum(axis=-3) / m0)
        var = (cube * (v - mean[..., None, :, :]) ** 2).sum(axis=-3) / m0
        sigma = np.where(m0 == 0., np.nan, np.sqrt(np.maximum(var, 0.)))
    return m0, mean, sigma


# the constants of the continuum images (csrc/device_common.h)
PLANCK = 6.626070040e-34
BOLTZMANN = 1.38064852e-23
LIGHTSPEED = 299792458.


def planck_function(nu, T):
    """B_nu(T) = 2 h nu^3 / c^2 / expm1(h nu / (k T)) in W m^-2 Hz^-1 sr^-1;
    0 for T <= 0. nu (Hz) and T (K) broadcast."""
    nu, T = np.broadcast_arrays(np.asarray(nu, dtype=np.float64),
                                np.asarray(T, dtype=np.float64))
    out = np.zeros(nu.shape)
    ok = T > 0.
    with np.errstate(over="ignore"):
        out[ok] = (2. * PLANCK * nu[ok] * nu[ok] * nu[ok] /
                   (LIGHTSPEED * LIGHTSPEED)) / \
            np.expm1((PLANCK * nu[ok]) / (BOLTZMANN * T[ok]))
    return out if out.ndim else float(out)


def brightness_temperature(I, nu):
    """The Rayleigh-Jeans brightness temperature c^2 I / (2 k nu^2) (K) of
    the specific intensity I (W m^-2 Hz^-1 sr^-1) at nu (Hz). With I of shape
    (nf, ...) and nu of shape (nf,) the frequencies go with the first axis."""
    I = np.asarray(I, dtype=np.float64)
    nu = np.asarray(nu, dtype=np.float64)
    if nu.ndim == 1 and I.ndim > 1:
        nu = nu.reshape((-1,) + (1,) * (I.ndim - 1))
    return LIGHTSPEED * LIGHTSPEED * I / (2. * BOLTZMANN * nu * nu)


def continuum_spectral_index(I, freq):
    """The slope of log I against log nu between neighbouring frequencies,
    per pixel: (nf - 1, ...) from I of shape (nf, ...) and freq[nf]; NaN
    where either intensity is not positive. -0.1 for thin free-free emission,
    2 for thick."""
    I = np.asarray(I, dtype=np.float64)
    nu = np.asarray(freq, dtype=np.float64).reshape(-1)
    if len(nu) != I.shape[0] or len(nu) < 2:
        raise ValueError("continuum_spectral_index needs I[nf][...] and "
                         "freq[nf], nf >= 2")
    dlognu = np.log(nu[1:] / nu[:-1]).reshape((-1,) + (1,) * (I.ndim - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (I[1:] > 0.) & (I[:-1] > 0.)
        ratio = np.where(ok, I[1:] / np.where(ok, I[:-1], 1.), np.nan)
        return np.log(ratio) / dlognu


def continuum_flux_density(I, pixel_solid_angle):
    """The flux density (W m^-2 Hz^-1; 1e26 of them are a jansky) per
    channel: the sum over the pixels of I (nf, nx, ny) times their solid
    angle (a scalar, or (nx, ny) as from sky_map_directions)."""
    I = np.asarray(I, dtype=np.float64)
    w = np.asarray(pixel_solid_angle, dtype=np.float64)
    return (I * w).reshape(I.shape[0], -1).sum(axis=1)


# the 21-cm line of the absorbing line cubes (csrc/absorbing_cube_kernels.h,
# csrc/device_common.h): the hyperfine frequency (Hz), its Einstein A (s^-1)
# and C_HI = 3 h c^3 A_10 / (32 pi k_B nu_10^2) in K m^3 s^-1
HI_FREQUENCY = 1420405751.768
HI_EINSTEIN_A = 2.8843e-15
HI_COLUMN_CONSTANT = 5.516606267115072e-20

# how the spin temperature of the H I calls is given
HI_SPIN_KINETIC, HI_SPIN_FIXED, HI_SPIN_CELLS = 0, 1, 2


def hi_column_density(cube, dv):
    """The H I column density (m^-2) of the optically thin limit from an H I
    cube (nchan, ...) in W m^-2 Hz^-1 sr^-1 with channels of dv m s^-1: the
    sum over the channels of the Rayleigh-Jeans brightness temperature times
    dv, over HI_COLUMN_CONSTANT. 1e-4 of it is the column in cm^-2."""
    T_b = brightness_temperature(np.asarray(cube, dtype=np.float64),
                                 HI_FREQUENCY)
    return T_b.sum(axis=0) * dv / HI_COLUMN_CONSTANT


_lib = None


def load_library():
    """Load libcmi_gpu.so (built by __graft_entry__.build()); no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            "HIP engine library not found at %s - build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C cmacionize_amd/csrc`. There is no CPU fallback." %
            LIB_PATH)
    # torch ships its own copy of the HIP runtime; if the engine's library
    # pulls in the system one first, torch cannot initialise the GPU later in
    # the same process. Let torch (the owner of streams and of the buffers it
    # shares with the engine) come first when it is there.
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.cmi_gpu_last_error.restype = C.c_char_p
    L.cmi_gpu_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.cmi_gpu_destroy.argtypes = [vp]
    L.cmi_gpu_synchronize.argtypes = [vp]
    L.cmi_gpu_number_of_cells.restype = C.c_int64
    L.cmi_gpu_number_of_cells.argtypes = [vp]
    L.cmi_gpu_set_sources.argtypes = [vp, C.c_int32, _dp, _dp, C.c_double]
    L.cmi_gpu_set_spectrum_monochromatic.argtypes = [vp, C.c_double]
    L.cmi_gpu_set_spectrum_planck.argtypes = [vp, C.c_double]
    L.cmi_gpu_set_continuous_source.argtypes = [vp, C.c_int32, C.c_double]
    L.cmi_gpu_set_continuous_source_planar.argtypes = [
        vp, C.c_int32, C.c_double, _dp, _dp, C.c_double]
    L.cmi_gpu_set_continuous_spectrum_monochromatic.argtypes = [vp, C.c_double]
    L.cmi_gpu_set_continuous_spectrum_planck.argtypes = [vp, C.c_double]
    L.cmi_gpu_set_cross_sections_fixed.argtypes = [vp, _dp]
    L.cmi_gpu_set_spectrum_table.argtypes = [vp, C.c_int32, C.c_int32, _dp,
                                             _dp, C.c_int32]
    L.cmi_gpu_set_cross_sections_table.argtypes = [vp, C.c_int32, _dp, _dp,
                                                   C.c_int32]
    L.cmi_gpu_set_recombination_rates_table.argtypes = [vp, C.c_int32, _dp,
                                                        _dp, C.c_int32]
    L.cmi_gpu_set_cross_sections_verner.argtypes = [vp]
    L.cmi_gpu_set_recombination_rates_fixed.argtypes = [vp, _dp]
    L.cmi_gpu_set_recombination_rates_verner.argtypes = [vp]
    L.cmi_gpu_set_abundances.argtypes = [vp, _dp]
    L.cmi_gpu_set_reemission.argtypes = [vp, C.c_int32, C.c_double,
                                         C.c_double]
    L.cmi_gpu_set_temperature_params.argtypes = [
        vp, C.POINTER(TemperatureParams)]
    L.cmi_gpu_upload_cells.argtypes = [vp, _dp, _dp, _dp]
    L.cmi_gpu_upload_field.argtypes = [vp, C.c_int32, _dp]
    L.cmi_gpu_download_field.argtypes = [vp, C.c_int32, _dp]
    L.cmi_gpu_field_device_pointer.restype = C.c_void_p
    L.cmi_gpu_field_device_pointer.argtypes = [vp, C.c_int32]
    if hasattr(L, "cmi_gpu_get_update_state"):  # (as for the stamps below)
        L.cmi_gpu_get_update_state.argtypes = [vp] + 3 * [C.POINTER(C.c_int32)]
    if hasattr(L, "cmi_gpu_get_transport_plan"):
        L.cmi_gpu_get_transport_plan.argtypes = [vp] + 2 * [
            C.POINTER(C.c_int32)]
    if hasattr(L, "cmi_gpu_get_bundle_march"):
        L.cmi_gpu_get_bundle_march.argtypes = [vp, C.POINTER(C.c_int32)]
    if hasattr(L, "cmi_gpu_get_bundle_point"):
        L.cmi_gpu_get_bundle_point.argtypes = [vp, C.POINTER(C.c_int32)]
    # (a build from before the bucket order, loaded through CMI_GPU_LIBRARY
    # for a comparison, does not have them)
    if hasattr(L, "cmi_gpu_get_order_plan"):
        L.cmi_gpu_get_order_plan.argtypes = [vp] + 3 * [
            C.POINTER(C.c_int32)] + [C.POINTER(C.c_uint64)]
        L.cmi_gpu_order_packets.argtypes = [
            vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
            C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.cmi_gpu_reset_grid.argtypes = [vp]
    L.cmi_gpu_shoot.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64,
                                C.c_uint64]
    L.cmi_gpu_get_counters.argtypes = [vp, _dp, _dp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_update_cells.argtypes = [vp, C.c_uint32, C.c_double]
    L.cmi_gpu_emit_packets.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64,
                                       C.c_uint64, _dp, _dp, _dp, _dp, _dp]
    L.cmi_gpu_trace_packets.argtypes = [
        vp, C.c_uint64, _dp, _dp, _dp, _dp, _dp, C.c_int32,
        C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
        _dp]
    L.cmi_gpu_get_timing.argtypes = [vp, C.c_int32, _dp, C.POINTER(C.c_uint64),
                                     _dp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_get_kernel_timing.argtypes = [vp, _dp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_set_tuning.argtypes = [vp, C.c_char_p, C.c_int64]
    L.cmi_gpu_get_atomic_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    # (a build from before the stamps, loaded through CMI_GPU_LIBRARY for a
    # comparison, does not have it)
    if hasattr(L, "cmi_gpu_get_phase_clocks"):
        L.cmi_gpu_get_phase_clocks.argtypes = [vp, C.POINTER(C.c_uint64),
                                               C.c_int64,
                                               C.POINTER(C.c_int64)]
    L.cmi_gpu_get_wave_steps.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_set_export_buffer.argtypes = [vp, vp, C.c_uint64]
    L.cmi_gpu_get_export_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_reset_exports.argtypes = [vp]
    L.cmi_gpu_download_exports.argtypes = [vp, _dp, C.c_uint64,
                                           C.POINTER(C.c_uint64)]
    L.cmi_gpu_shoot_flights_host.argtypes = [vp, C.c_uint32, C.c_uint32,
                                             C.c_uint64, _dp, C.c_uint64]
    L.cmi_gpu_shoot_flights.argtypes = [vp, C.c_uint32, C.c_uint32,
                                        C.c_uint64, vp, C.c_uint64]
    L.cmi_gpu_get_launch_times.argtypes = [vp, C.c_uint64, _dp,
                                           C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]
    L.cmi_gpu_sample_spectrum.argtypes = [vp, C.c_int32, C.c_double,
                                          C.c_uint32, C.c_uint64, _dp]
    L.cmi_gpu_accumulator_layout.argtypes = [vp, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]
    L.cmi_gpu_thermal_probe.argtypes = [vp, C.c_int64, C.c_int32, _dp, _dp,
                                        _dp, _dp, _dp, _dp, _dp]
    L.cmi_gpu_physics_probe.argtypes = [vp, C.c_int32, C.c_int64, _dp, _dp]
    L.cmi_gpu_compute_emissivities.argtypes = [
        vp, C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.c_int64,
        C.POINTER(C.c_double)]
    L.cmi_gpu_set_spectrum_trackers.argtypes = [vp, C.c_int32, _dp, C.c_int32,
                                                _dp, _dp]
    L.cmi_gpu_set_trackers.argtypes = [vp, C.c_int32, _dp,
                                       C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), _dp, _dp]
    L.cmi_gpu_get_tracker_absorption.argtypes = [vp, _dp]
    L.cmi_gpu_enable_trackers.argtypes = [vp, C.c_int32]
    L.cmi_gpu_set_tracker_frequency_bins.argtypes = [
        vp, C.c_int32, C.c_int32, C.c_double, C.c_double]
    L.cmi_gpu_get_tracker_flux.argtypes = [vp, _dp]
    L.cmi_gpu_projected_areas.argtypes = [_dp, C.c_int64, _dp]
    L.cmi_gpu_get_tracker_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_set_escape_tally.argtypes = [
        vp, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_int32, C.c_double,
        C.c_double]
    L.cmi_gpu_reset_escape_tally.argtypes = [vp]
    L.cmi_gpu_download_escape_tally.argtypes = [vp, _dp]
    L.cmi_gpu_escape_pixels.argtypes = [_dp, C.c_int32, C.c_int32, C.c_int64,
                                        _dp, C.POINTER(C.c_int32), _dp]
    L.cmi_gpu_cross_sections.argtypes = [vp, C.c_int64, _dp, _dp]
    L.cmi_gpu_sph_map_to_cells.argtypes = [
        vp, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, _dp, _dp, _dp, _dp,
        C.POINTER(C.c_int32), _dp]
    L.cmi_gpu_sph_map_to_particles.argtypes = [
        vp, C.c_int32, C.c_int64, _dp, _dp, _dp, _dp, _dp,
        C.POINTER(C.c_int32), _dp, _dp]
    L.cmi_gpu_get_sph_map_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    L.cmi_gpu_update_cells_range.argtypes = [vp, C.c_uint32, C.c_double,
                                             C.c_int64, C.c_int64]
    L.cmi_gpu_refresh_transport_records.argtypes = [vp]
    L.cmi_gpu_get_launch_steps.argtypes = [vp, C.c_uint64,
                                           C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]
    L.cmi_gpu_group_create.argtypes = [C.c_int32, C.POINTER(vp),
                                       C.POINTER(vp)]
    L.cmi_gpu_group_destroy.argtypes = [vp]
    L.cmi_gpu_group_reduce_accumulators.argtypes = [vp]
    L.cmi_gpu_group_update_cells.argtypes = [vp, C.c_uint32, C.c_double]
    L.cmi_gpu_group_exchange_flights.argtypes = [
        vp, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.cmi_gpu_group_exchange_stats.argtypes = [
        vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_int32]
    L.cmi_gpu_set_dust_scattering.argtypes = [vp, C.c_double, C.c_double,
                                              C.c_double, C.c_double]
    L.cmi_gpu_set_ccd_image.argtypes = [vp, C.c_double, C.c_double, C.c_int32,
                                        C.c_int32, _dp, _dp]
    L.cmi_gpu_set_continuous_source_spiral_galaxy.argtypes = [
        vp, C.c_double, C.c_double, C.c_double]
    L.cmi_gpu_dust_shoot.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64]
    L.cmi_gpu_download_image.argtypes = [vp, _dp, _dp, _dp]
    L.cmi_gpu_reset_image.argtypes = [vp]
    L.cmi_gpu_get_dust_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_dust_probe.argtypes = [vp, C.c_int32, C.c_uint32, C.c_uint64,
                                     C.c_int64, _dp, _dp, C.c_int32]
    L.cmi_gpu_render_line_images.argtypes = [
        vp, C.c_int32, C.POINTER(C.c_int32), C.c_double, C.c_double,
        C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_double, _dp]
    L.cmi_gpu_render_field_images.argtypes = [
        vp, C.c_int32, _dp, C.c_double, C.c_double, C.c_int32, C.c_int32, _dp,
        _dp, C.c_int32, _dp, _dp]
    L.cmi_gpu_set_cell_velocities.argtypes = [vp, _dp]
    L.cmi_gpu_emission_line_atomic_weight.argtypes = [C.c_int32]
    L.cmi_gpu_emission_line_atomic_weight.restype = C.c_double
    L.cmi_gpu_render_line_cube.argtypes = [
        vp, C.c_int32, C.POINTER(C.c_int32), C.c_double, C.c_double,
        C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_double, C.c_int32,
        C.c_double, C.c_double, C.c_double, _dp]
    L.cmi_gpu_render_field_cube.argtypes = [
        vp, C.c_int32, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int32,
        C.c_int32, _dp, _dp, C.c_int32, C.c_int32, C.c_double, C.c_double,
        _dp]
    L.cmi_gpu_set_dust_scattering_per_hydrogen.argtypes = [
        vp, C.c_double, C.c_double, C.c_double, C.c_double]
    L.cmi_gpu_set_cell_source_line.argtypes = [vp, C.c_int32]
    L.cmi_gpu_set_cell_source_field.argtypes = [vp, _dp]
    L.cmi_gpu_get_cell_source.argtypes = [vp, _dp, _dp, _dp]
    L.cmi_gpu_line_image_probe.argtypes = [vp, C.c_double, C.c_double,
                                           C.c_int64, _dp, C.c_int32, _dp]
    L.cmi_gpu_render_line_sky.argtypes = [
        vp, C.c_int32, C.POINTER(C.c_int32), _dp, C.c_int64, _dp, C.c_double,
        _dp]
    L.cmi_gpu_render_field_sky.argtypes = [
        vp, C.c_int32, _dp, _dp, C.c_int64, _dp, _dp, _dp]
    L.cmi_gpu_sky_probe.argtypes = [vp, _dp, C.c_int64, _dp, C.c_int32, _dp]
    L.cmi_gpu_render_line_sky_map.argtypes = [
        vp, C.c_int32, C.POINTER(C.c_int32), _dp, _dp, C.c_double, C.c_double,
        C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, _dp]
    L.cmi_gpu_render_field_sky_cube.argtypes = [
        vp, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int64, _dp,
        C.c_int32, C.c_double, C.c_double, _dp]
    L.cmi_gpu_render_line_sky_cube.argtypes = [
        vp, C.c_int32, C.POINTER(C.c_int32), _dp, _dp, C.c_int64, _dp,
        C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, _dp]
    L.cmi_gpu_render_line_sky_map_cube.argtypes = [
        vp, C.c_int32, C.POINTER(C.c_int32), _dp, _dp, C.c_double, C.c_double,
        C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, _dp,
        C.c_int32, C.c_double, C.c_double, C.c_double, _dp]
    L.cmi_gpu_sky_map_directions.argtypes = [
        _dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32,
        C.c_int32, _dp, _dp]
    L.cmi_gpu_set_sky_camera.argtypes = [
        vp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double,
        C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.cmi_gpu_check_sky_camera.argtypes = [
        _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double,
        C.c_int32, C.c_int32, C.c_double]
    L.cmi_gpu_get_sky_camera_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cmi_gpu_set_ccd_images.argtypes = [vp, C.c_int32, _dp, _dp, C.c_int32,
                                         C.c_int32, _dp, _dp]
    L.cmi_gpu_set_sky_cameras.argtypes = [
        vp, C.c_int32, _dp, _dp, C.c_double, C.c_double, C.c_double,
        C.c_double, C.c_int32, C.c_int32, _dp, C.c_int32]
    L.cmi_gpu_download_image_view.argtypes = [vp, C.c_int32, _dp, _dp, _dp]
    L.cmi_gpu_get_dust_view_counters.argtypes = [vp, C.c_int32,
                                                 C.POINTER(C.c_uint64)]
    L.cmi_gpu_select_probe_view.argtypes = [vp, C.c_int32]
    L.cmi_gpu_set_scattered_cube.argtypes = [
        vp, C.c_int32, C.c_double, C.c_double, C.c_double, _dp, _dp]
    L.cmi_gpu_download_cube_view.argtypes = [vp, C.c_int32, _dp, _dp, _dp]
    # (a build from before Lyman alpha, loaded through CMI_GPU_LIBRARY for a
    # comparison, does not have it)
    if hasattr(L, "cmi_gpu_set_lyman_alpha"):
        L.cmi_gpu_set_lyman_alpha.argtypes = [
            vp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
            C.c_uint64, _dp, _dp]
        L.cmi_gpu_lya_shoot.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64]
        L.cmi_gpu_lya_probe.argtypes = [vp, C.c_int32, C.c_uint32, C.c_uint64,
                                        C.c_int64, _dp, _dp, C.c_int32]
        L.cmi_gpu_download_lya_view.argtypes = [vp, C.c_int32, _dp, _dp]
        L.cmi_gpu_reset_lya.argtypes = [vp]
        L.cmi_gpu_get_lya_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.cmi_gpu_lyman_alpha_emissivity.argtypes = [vp, _dp]
    # (nor does a build from before the Lyman-alpha radiation field have it)
    if hasattr(L, "cmi_gpu_set_lya_field"):
        L.cmi_gpu_set_lya_field.argtypes = [vp, C.c_int32]
        L.cmi_gpu_download_lya_field.argtypes = [vp, _dp]
        L.cmi_gpu_lya_spin_temperature.argtypes = [
            vp, C.c_double, C.c_double, C.c_int32, _dp, _dp]
    # (a build from before the continuum images, loaded through
    # CMI_GPU_LIBRARY for a comparison, does not have them)
    if hasattr(L, "cmi_gpu_free_free_coefficients"):
        L.cmi_gpu_free_free_coefficients.argtypes = [vp, C.c_int32, _dp,
                                                     _dp, _dp]
        L.cmi_gpu_render_continuum_images.argtypes = [
            vp, C.c_int32, _dp, _dp, C.c_double, C.c_double, C.c_int32, C.c_int32,
            _dp, _dp, C.c_int32, _dp]
        L.cmi_gpu_render_field_continuum_images.argtypes = [
            vp, C.c_int32, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int32,
            C.c_int32, _dp, _dp, C.c_int32, _dp]
        L.cmi_gpu_render_continuum_sky.argtypes = [
            vp, C.c_int32, _dp, _dp, _dp, C.c_int64, _dp, _dp]
        L.cmi_gpu_render_field_continuum_sky.argtypes = [
            vp, C.c_int32, _dp, _dp, _dp, _dp, C.c_int64, _dp, _dp]
        L.cmi_gpu_render_continuum_sky_map.argtypes = [
            vp, C.c_int32, _dp, _dp, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp,
            _dp]
        L.cmi_gpu_continuum_probe.argtypes = [
            vp, C.c_int32, _dp, _dp, _dp, C.c_int32, _dp, C.c_int64, _dp,
            C.c_int32, _dp]
    # (likewise a build from before the absorbing line cubes)
    if hasattr(L, "cmi_gpu_hi_coefficients"):
        hi = [C.c_double, C.c_int32, _dp, C.c_int32]
        axis = [C.c_int32, C.c_double, C.c_double]
        L.cmi_gpu_hi_coefficients.argtypes = [vp] + hi + [_dp] * 5
        L.cmi_gpu_render_hi_cube.argtypes = [
            vp, C.c_double, C.c_double, C.c_int32, C.c_int32, _dp, _dp,
            C.c_int32] + axis + hi + [C.c_double, _dp]
        L.cmi_gpu_render_hi_sky_cube.argtypes = [
            vp, _dp, _dp, C.c_int64, _dp] + axis + hi + [C.c_double, _dp]
        L.cmi_gpu_render_hi_sky_map_cube.argtypes = [
            vp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double,
            C.c_int32, C.c_int32, _dp] + axis + hi + [C.c_double, _dp]
        L.cmi_gpu_render_field_absorbing_cube.argtypes = [
            vp] + [_dp] * 7 + [C.c_double, C.c_double, C.c_int32, C.c_int32,
                               _dp, _dp, C.c_int32] + axis + [_dp]
        L.cmi_gpu_render_field_absorbing_sky_cube.argtypes = [
            vp] + [_dp] * 7 + [_dp, _dp, C.c_int64, _dp] + axis + [_dp]
        L.cmi_gpu_absorbing_cube_probe.argtypes = [
            vp] + [_dp] * 7 + axis + [C.c_int32, _dp, _dp, C.c_int64, _dp,
                                      C.c_int32, _dp]
    # (nor does a build from before the absorption spectra have them)
    if hasattr(L, "cmi_gpu_render_field_absorption_spectra"):
        ip = C.POINTER(C.c_int32)
        axis = [C.c_int32, C.c_double, C.c_double]
        sightlines = [C.c_int64, _dp, _dp, _dp, _dp]
        L.cmi_gpu_render_field_absorption_spectra.argtypes = [
            vp, C.c_int32, _dp, _dp, _dp, _dp, _dp] + sightlines + axis + [
                _dp, _dp]
        L.cmi_gpu_render_absorption_spectra.argtypes = [
            vp, C.c_int32, ip, _dp, _dp, _dp, C.c_double] + sightlines + \
            axis + [_dp, _dp]
        L.cmi_gpu_absorption_probe.argtypes = [
            vp, _dp, _dp, C.c_double, C.c_double, _dp, _dp, _dp, C.c_double,
            _dp] + axis + [C.c_int32, ip, C.c_int32, _dp]
    _lib = L
    return L


# physical constants of the absorption lines (SI, CODATA 2018)
_ELEMENTARY_CHARGE = 1.602176634e-19
_VACUUM_PERMITTIVITY = 8.8541878128e-12
_ELECTRON_MASS = 9.1093837015e-31
_LIGHTSPEED = 299792458.

# The ions the engine tracks, in the order of its ionic fractions.
ION_NAMES = ("H0", "He0", "C+", "C2+", "N0", "N+", "N2+", "O0", "O+", "Ne0",
             "Ne+", "S+", "S2+", "S3+")
_ION_ELEMENTS = ("H", "He", "C", "C", "N", "N", "N", "O", "O", "Ne", "Ne",
                 "S", "S", "S")

# One resonance line per tracked ion: name -> (ion index, vacuum wavelength in
# m, oscillator strength f, damping constant Gamma in s^-1). Wavelengths and f
# values after Morton (2003, ApJS 149, 205) where that compilation has the
# line and the NIST Atomic Spectra Database otherwise, rounded to the figures
# given; Gamma is the sum of the upper level's transition probabilities as
# NIST lists them, to two or three figures. H I carries the literals of the
# Lyman-alpha transfer (CMI_LYA_LAMBDA0, CMI_LYA_A21), so that a = g / b is
# that mode's. The other rows have not been checked against the two sources
# entry by entry ("Not measured"): work that depends on a
# line's f or Gamma should pass its own constants to
# absorption_line_constants.
ABSORPTION_LINES = {
    "HI_1215": (0, LYA_LAMBDA0, 0.4164, 6.265e8),
    "HeI_584": (1, 584.334e-10, 0.2763, 1.799e9),
    "CII_1334": (2, 1334.532e-10, 0.1278, 2.88e8),
    "CIII_977": (3, 977.020e-10, 0.7570, 1.767e9),
    "NI_1199": (4, 1199.550e-10, 0.1320, 4.07e8),
    "NII_1083": (5, 1083.994e-10, 0.1110, 3.74e8),
    "NIII_989": (6, 989.799e-10, 0.1230, 5.00e8),
    "OI_1302": (7, 1302.168e-10, 0.0480, 5.65e8),
    "OII_834": (8, 834.466e-10, 0.1320, 8.60e8),
    "NeI_735": (9, 735.896e-10, 0.1590, 6.11e8),
    "NeII_460": (10, 460.728e-10, 0.0900, 7.00e9),
    "SII_1259": (11, 1259.518e-10, 0.0166, 4.65e7),
    "SIII_1190": (12, 1190.203e-10, 0.0237, 6.70e7),
    "SIV_1062": (13, 1062.664e-10, 0.0494, 1.60e8),
}


def absorption_line_constants(wavelength, f, gamma):
    """(S, g) of a line of rest wavelength `wavelength` (m), oscillator
    strength f and damping constant gamma (s^-1): the cross section
    integrated over velocity S = e^2 f lambda0 / (4 eps0 m_e c), m^2 m s^-1,
    and the damping width g = gamma lambda0 / (4 pi), m s^-1
    (include/cmi_gpu.h, "absorption spectra")."""
    S = (_ELEMENTARY_CHARGE * _ELEMENTARY_CHARGE * f * wavelength /
         (4. * _VACUUM_PERMITTIVITY * _ELECTRON_MASS * _LIGHTSPEED))
    return S, gamma * wavelength / (4. * np.pi)


def transmitted_flux(tau):
    """exp(-tau): the flux of a background source of unit continuum."""
    return np.exp(-np.asarray(tau, dtype=np.float64))


def equivalent_width(tau, dv, wavelength):
    """The equivalent width (m) of spectra tau[..., nchan] of channel width
    dv (m s^-1): (lambda0 / c) sum_c (1 - exp(-tau_c)) dv."""
    tau = np.asarray(tau, dtype=np.float64)
    return (wavelength / _LIGHTSPEED) * (-np.expm1(-tau)).sum(axis=-1) * dv


def apparent_column_density(tau, dv, S):
    """The apparent column density (m^-2) of spectra tau[..., nchan]: sum_c
    tau_c dv / S, the true one where the line is resolved."""
    return np.asarray(tau, dtype=np.float64).sum(axis=-1) * dv / S


def absorption_table_lines(names):
    """(ions, weights, S, g, wavelengths) of entries of ABSORPTION_LINES."""
    rows = [ABSORPTION_LINES[n] for n in names]
    Sg = [absorption_line_constants(w, f, gamma) for _, w, f, gamma in rows]
    return (np.array([r[0] for r in rows], dtype=np.int32),
            np.array([_ELEMENT_WEIGHTS[_ION_ELEMENTS[r[0]]] for r in rows]),
            np.array([s for s, _ in Sg]), np.array([g for _, g in Sg]),
            np.array([r[1] for r in rows]))


def projected_areas(directions):
    """WeightedSpectrumTracker::get_projected_area of unit vectors ([n][3]),
    by the function the kernels call, run on the host"""
    d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(d))
    rc = load_library().cmi_gpu_projected_areas(_p(d), len(d), _p(out))
    if rc != 0:
        raise RuntimeError("cmi_gpu_projected_areas failed (%d)" % rc)
    return out


FULL_SKY_LONGITUDE = (-np.pi, np.pi)
FULL_SKY_LATITUDE = (-0.5 * np.pi, 0.5 * np.pi)
IDENTITY_FRAME = ((1., 0., 0.), (0., 1., 0.), (0., 0., 1.))


def sky_map_directions(nlon, nlat, lon_range=FULL_SKY_LONGITUDE,
                       lat_range=FULL_SKY_LATITUDE, frame=IDENTITY_FRAME):
    """The rays of an equirectangular map (include/cmi_gpu.h, "sky maps"), by
    the function cmi_gpu_render_line_sky_map calls, run on the host: the
    directions (nlon * nlat, 3) of the pixel centres in pixel order - pixel
    (i, j) at i * nlat + j - and the exact solid angles dl (sin b_hi -
    sin b_lo) of the pixels, so that a flux is sum(I * omega). Radians; the
    rows of `frame` are e_1 (l = 0, b = 0), e_2 (l = 90 deg) and e_3 (the
    pole). Users of other pixelisations (HEALPix's pix2vec) pass their own
    unit vectors to GpuEngine.render_line_sky."""
    f = _f64(frame).reshape(9)
    n = max(int(nlon), 0) * max(int(nlat), 0)
    d = np.zeros((n, 3))
    omega = np.zeros(n)
    L = load_library()
    rc = L.cmi_gpu_sky_map_directions(
        _p(f), lon_range[0], lon_range[1], lat_range[0], lat_range[1],
        int(nlon), int(nlat), _p(d), _p(omega))
    if rc != 0:
        raise EngineError(L.cmi_gpu_last_error().decode())
    return d, omega


def sky_frame(pole=(0., 0., 1.), zero_longitude=(1., 0., 0.)):
    """The frame ((e_1, e_2, e_3) as rows) of a pole and a zero of longitude,
    orthonormalised as the driver's EmissionSkyMaps block does: the pole is
    kept, the zero of longitude is made perpendicular to it, e_2 = e_3 x e_1.
    The default pole gives e_3 = (0, 0, 1) exactly."""
    e3 = np.asarray(pole, dtype=np.float64)
    zero = np.asarray(zero_longitude, dtype=np.float64)
    e3 = e3 / np.sqrt(e3 @ e3)
    e1 = zero - (zero @ e3) * e3
    norm = np.sqrt(e1 @ e1)
    if not norm > 1e-8 * np.sqrt(zero @ zero):
        raise ValueError("the frame's pole and zero of longitude are parallel")
    e1 = e1 / norm
    return np.array([e1, np.cross(e3, e1), e3])


def escape_pixels(directions, nlon, nmu, frame=IDENTITY_FRAME):
    """The escape tally's pixel i * nmu + j of unit vectors ([n][3]), by the
    function the transport kernels call, run on the host (include/cmi_gpu.h,
    "escape maps")."""
    d = _f64(directions).reshape(-1, 3)
    out = np.zeros(len(d), dtype=np.int32)
    L = load_library()
    rc = L.cmi_gpu_escape_pixels(
        _p(_f64(frame).reshape(9)), int(nlon), int(nmu), len(d), _p(d),
        out.ctypes.data_as(C.POINTER(C.c_int32)), None)
    if rc != 0:
        raise EngineError("cmi_gpu error %d: %s" % (
            rc, L.cmi_gpu_last_error().decode()))
    return out


def escape_pixel_centres(nlon, nmu, frame=IDENTITY_FRAME):
    """The unit vectors (nlon, nmu, 3) of the escape tally's pixel centres."""
    out = np.zeros((int(nlon), int(nmu), 3))
    L = load_library()
    rc = L.cmi_gpu_escape_pixels(
        _p(_f64(frame).reshape(9)), int(nlon), int(nmu), 0, None, None,
        _p(out))
    if rc != 0:
        raise EngineError("cmi_gpu error %d: %s" % (
            rc, L.cmi_gpu_last_error().decode()))
    return out


def escape_fraction_map(tally, totweight):
    """The escaping luminosity per steradian in units of L / 4 pi, (nlon,
    nmu): an escape tally (3, nfreq, nlon, nmu) summed over types and bins,
    times the number of pixels over the total weight of the packets. Its mean
    is the escape fraction."""
    t = np.asarray(tally, dtype=np.float64)
    return t.sum(axis=(0, 1)) * (t.shape[2] * t.shape[3]) / totweight


def escape_spectrum(tally, totweight, luminosity):
    """Escaping photons s^-1 per type and frequency bin, (3, nfreq), of a
    source of `luminosity` photons s^-1."""
    t = np.asarray(tally, dtype=np.float64)
    return t.sum(axis=(2, 3)) * (luminosity / totweight)


def check_sky_camera(box_anchor, box_sides, origin, nlon, nlat,
                     exclusion_radius, lon_range=FULL_SKY_LONGITUDE,
                     lat_range=FULL_SKY_LATITUDE, frame=IDENTITY_FRAME):
    """GpuEngine.set_sky_camera's argument checks for a box, run on the host
    (cmi_gpu_check_sky_camera): raises EngineError as that call would."""
    L = load_library()
    rc = L.cmi_gpu_check_sky_camera(
        _p(_f64(box_anchor).reshape(3)), _p(_f64(box_sides).reshape(3)),
        _p(_f64(origin).reshape(3)), _p(_f64(frame).reshape(9)),
        lon_range[0], lon_range[1], lat_range[0], lat_range[1], int(nlon),
        int(nlat), exclusion_radius)
    if rc != 0:
        raise EngineError("cmi_gpu error %d: %s" % (
            rc, L.cmi_gpu_last_error().decode()))


def _p(a):
    return a.ctypes.data_as(_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p_or_none(a):
    """_p(a), and the null pointer for None."""
    return None if a is None else _p(a)


def _line_indices(names):
    """The indices in EMISSION_LINES of `names` as the int32 pointer the
    library takes (it keeps its array alive)."""
    idx = np.array([EMISSION_LINES.index(n) for n in names], dtype=np.int32)
    return idx.ctypes.data_as(C.POINTER(C.c_int32))


class EngineGroup:
    """Several engines driven by this process (cmi_gpu_group_*): replicas
    (reduce_accumulators) or the blocks of a decomposed grid
    (exchange_flights)."""

    def __init__(self, engines):
        self._lib = load_library()
        self.engines = list(engines)
        handles = (C.c_void_p * len(self.engines))(
            *[e._h for e in self.engines])
        self._h = C.c_void_p()
        rc = self._lib.cmi_gpu_group_create(len(self.engines), handles,
                                            C.byref(self._h))
        if rc != 0:
            raise EngineError(self._lib.cmi_gpu_last_error().decode())

    def _check(self, rc):
        if rc != 0:
            raise EngineError(self._lib.cmi_gpu_last_error().decode())

    def reduce_accumulators(self):
        self._check(self._lib.cmi_gpu_group_reduce_accumulators(self._h))

    def update_cells(self, loop, totweight):
        """Sharded cell update of every class of the group (slab r solved
        by member r, then gathered into every member)."""
        self._check(self._lib.cmi_gpu_group_update_cells(self._h, loop,
                                                         totweight))

    def exchange_flights(self, seed, iteration, first_packet=0):
        total = C.c_uint64()
        self._check(self._lib.cmi_gpu_group_exchange_flights(
            self._h, seed, iteration, first_packet, C.byref(total)))
        return total.value

    def exchange_stats(self, reset=True):
        """Host-side cost of the exchange rounds since the last reset:
        {rounds, counts_us, threads_us, total_us} (sums over the rounds)."""
        rounds = C.c_uint64()
        us = (C.c_double * 3)()
        self._check(self._lib.cmi_gpu_group_exchange_stats(
            self._h, C.byref(rounds), us, 1 if reset else 0))
        return dict(rounds=rounds.value, counts_us=us[0], threads_us=us[1],
                    total_us=us[2])

    def close(self):
        if self._h:
            self._lib.cmi_gpu_group_destroy(self._h)
            self._h = C.c_void_p()


class GpuEngine:
    """One engine handle = one grid on one GPU."""

    def __init__(self, ncell, anchor, sides, periodic=(0, 0, 0), device=0,
                 track_heating=False, stream=None, external_accumulators=None,
                 sub_offset=None, sub_ncell=None):
        """ncell/anchor/sides describe the whole grid; sub_offset/sub_ncell
        make the engine hold one block of it (domain decomposition)."""
        self._lib = load_library()
        cfg = Config()
        if sub_ncell is not None:
            for a in range(3):
                cfg.sub_offset[a] = int(sub_offset[a])
                cfg.sub_ncell[a] = int(sub_ncell[a])
        for a in range(3):
            cfg.anchor[a] = anchor[a]
            cfg.sides[a] = sides[a]
            cfg.ncell[a] = int(ncell[a])
            cfg.periodic[a] = int(bool(periodic[a]))
        cfg.device = device
        cfg.track_heating = int(bool(track_heating))
        cfg.stream = stream
        cfg.external_accumulators = external_accumulators
        self._h = C.c_void_p()
        self._check(self._lib.cmi_gpu_create(C.byref(cfg), C.byref(self._h)))
        self.ncell = tuple(int(n) for n in
                           (sub_ncell if sub_ncell is not None else ncell))
        self.n = int(np.prod(self.ncell))
        self.cube_channels = 0  # set_scattered_cube's nchan; 0: off
        self.lya_channels = 0  # set_lyman_alpha's nchan; 0: off
        self.lya_x_crit = 0.
        self._abundances = np.zeros(6)  # He, C, N, O, Ne, S per hydrogen
        self._escape = None  # set_escape_tally's (nfreq, nlon, nmu)
        # the whole grid, the default grid of the SPH mappings
        self._grid = (tuple(float(a) for a in anchor),
                      tuple(float(s) for s in sides),
                      tuple(int(n) for n in ncell))
        self.cell_volume = float(np.prod([float(sides[a]) / int(ncell[a])
                                          for a in range(3)]))  # m^3
        # tests, bench and tools read device timings; the engine records them
        # only on request
        self.set_tuning(timing=1)

    def _check(self, rc):
        if rc != 0:
            raise EngineError("cmi_gpu error %d: %s" % (
                rc, self._lib.cmi_gpu_last_error().decode()))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.cmi_gpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # plugin descriptors -----------------------------------------------------
    def set_sources(self, positions, weights, luminosity):
        w = _f64(weights)
        if len(w) == 0:  # no discrete sources
            self._check(self._lib.cmi_gpu_set_sources(self._h, 0, None, None,
                                                      0.))
            return
        pos = _f64(positions).reshape(-1, 3)
        self._check(self._lib.cmi_gpu_set_sources(self._h, len(w), _p(pos),
                                                  _p(w), luminosity))

    def set_continuous_source(self, kind, luminosity):
        """ContinuousPhotonSource (CONTINUOUS_ISOTROPIC on the box) with the
        luminosity the PhotonSource ctor computes for it."""
        self._check(self._lib.cmi_gpu_set_continuous_source(self._h, kind,
                                                            luminosity))

    def set_continuous_source_planar(self, axis, intercept, anchor, sides,
                                     luminosity):
        """PlanarContinuousPhotonSource: the rectangle [anchor, anchor +
        sides] of the plane x[axis] = intercept."""
        a = _f64(anchor)
        s = _f64(sides)
        self._check(self._lib.cmi_gpu_set_continuous_source_planar(
            self._h, axis, intercept, _p(a), _p(s), luminosity))

    def set_continuous_spectrum_monochromatic(self, frequency):
        self._check(self._lib.cmi_gpu_set_continuous_spectrum_monochromatic(
            self._h, frequency))

    def set_continuous_spectrum_planck(self, temperature):
        self._check(self._lib.cmi_gpu_set_continuous_spectrum_planck(
            self._h, temperature))

    def set_spectrum_monochromatic(self, frequency):
        self._check(self._lib.cmi_gpu_set_spectrum_monochromatic(self._h,
                                                                 frequency))

    def set_spectrum_planck(self, temperature):
        self._check(self._lib.cmi_gpu_set_spectrum_planck(self._h,
                                                          temperature))

    def set_spectrum_table(self, frequency, cumulative, role=ROLE_SOURCE,
                           interpolation=TABLE_LINEAR):
        """Generic lowering of a PhotonSourceSpectrum: its quantile function
        (cumulative[n] from 0 to 1 -> frequency[n] in Hz)."""
        f, c = _f64(frequency), _f64(cumulative)
        assert f.shape == c.shape and f.ndim == 1
        self._check(self._lib.cmi_gpu_set_spectrum_table(
            self._h, role, len(f), _p(f), _p(c), interpolation))

    def set_cross_sections_table(self, frequency, sigma,
                                 interpolation=TABLE_LINEAR):
        """Generic lowering of CrossSections: sigma[14][n] (m^2) on the
        frequencies frequency[n] (Hz)."""
        f, s = _f64(frequency), _f64(sigma)
        assert s.shape == (NION, len(f))
        self._check(self._lib.cmi_gpu_set_cross_sections_table(
            self._h, len(f), _p(f), _p(s), interpolation))

    def set_recombination_rates_table(self, temperature, alpha,
                                      interpolation=TABLE_LOGLOG):
        """Generic lowering of RecombinationRates: alpha[14][n] (m^3 s^-1) on
        the temperatures temperature[n] (K)."""
        t, a = _f64(temperature), _f64(alpha)
        assert a.shape == (NION, len(t))
        self._check(self._lib.cmi_gpu_set_recombination_rates_table(
            self._h, len(t), _p(t), _p(a), interpolation))

    def set_cross_sections_fixed(self, sigma):
        s = _f64(sigma)
        assert s.shape == (NION,)
        self._check(self._lib.cmi_gpu_set_cross_sections_fixed(self._h, _p(s)))

    def set_cross_sections_verner(self):
        self._check(self._lib.cmi_gpu_set_cross_sections_verner(self._h))

    def set_recombination_rates_fixed(self, alpha):
        a = _f64(alpha)
        assert a.shape == (NION,)
        self._check(self._lib.cmi_gpu_set_recombination_rates_fixed(self._h,
                                                                    _p(a)))

    def set_recombination_rates_verner(self):
        self._check(self._lib.cmi_gpu_set_recombination_rates_verner(self._h))

    def set_abundances(self, abundances):
        a = _f64(abundances)
        assert a.shape == (6,)
        self._check(self._lib.cmi_gpu_set_abundances(self._h, _p(a)))
        self._abundances = a.copy()

    def set_reemission(self, kind, probability=0., frequency=0.):
        self._check(self._lib.cmi_gpu_set_reemission(self._h, kind,
                                                     probability, frequency))

    def set_temperature_params(self, **kw):
        p = TemperatureParams(0, 3, 1.e-3, 100, 0., 0., 0.75,
                              1.33333 * 3.086e19, 4000.)
        for k, v in kw.items():
            setattr(p, k, v)
        self._check(self._lib.cmi_gpu_set_temperature_params(self._h,
                                                             C.byref(p)))

    # cell data --------------------------------------------------------------
    def upload_cells(self, number_density, temperature, ionic_fractions=None):
        n = _f64(number_density).ravel()
        t = _f64(temperature).ravel()
        assert n.size == self.n and t.size == self.n
        x = None
        if ionic_fractions is not None:
            x = _f64(ionic_fractions).reshape(NION, self.n)
        self._check(self._lib.cmi_gpu_upload_cells(
            self._h, _p(n), _p(t), _p_or_none(x)))

    def upload_field(self, field, values):
        v = _f64(values).ravel()
        assert v.size == self.n
        self._check(self._lib.cmi_gpu_upload_field(self._h, field, _p(v)))

    def download_field(self, field):
        out = np.empty(self.n)
        self._check(self._lib.cmi_gpu_download_field(self._h, field, _p(out)))
        return out

    def accumulator_layout(self):
        fs, cs = C.c_int64(), C.c_int64()
        self._check(self._lib.cmi_gpu_accumulator_layout(
            self._h, C.byref(fs), C.byref(cs)))
        return fs.value, cs.value

    def field_device_pointer(self, field):
        return self._lib.cmi_gpu_field_device_pointer(self._h, field)

    def update_state(self):
        """(x[2..13] of the last update still to be made, padded records
        valid, a whole-grid update may defer x[2..13]) as booleans."""
        v = [C.c_int32() for _ in range(3)]
        self._check(self._lib.cmi_gpu_get_update_state(
            self._h, *[C.byref(x) for x in v]))
        return tuple(bool(x.value) for x in v)

    def transport_plan(self):
        """(first-generation build, built for packets of one weight) of the
        last shoot: 0 the general kernel, 1 the block table, 2 / 3 the padded
        march in its smaller / larger blocks, 4 the multi-ion kernel with the
        emission physics done ahead."""
        first, uniform = C.c_int32(), C.c_int32()
        self._check(self._lib.cmi_gpu_get_transport_plan(
            self._h, C.byref(first), C.byref(uniform)))
        return first.value, bool(uniform.value)

    def bundle_march_flown(self):
        """Whether the first generation of the last shoot flew the bundle
        build of the padded march (tuning "bundle_march")."""
        flown = C.c_int32()
        self._check(self._lib.cmi_gpu_get_bundle_march(self._h,
                                                       C.byref(flown)))
        return bool(flown.value)

    def bundle_point_flown(self):
        """... and whether it was the point build of the bundle build: one
        discrete source, no continuous one (tuning "bundle_point")."""
        flown = C.c_int32()
        self._check(self._lib.cmi_gpu_get_bundle_point(self._h,
                                                       C.byref(flown)))
        return bool(flown.value)

    def order_plan(self):
        """(path, bits of the first scatter level, of the second, packets
        that overflowed) of the last launch of new packets: path ORDER_NONE,
        ORDER_RADIX (key kernel and radix sort) or ORDER_BUCKET (the bucket
        order, tuning "bucket_order")."""
        path, b1, b2 = C.c_int32(), C.c_int32(), C.c_int32()
        overflow = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_order_plan(
            self._h, C.byref(path), C.byref(b1), C.byref(b2),
            C.byref(overflow)))
        return path.value, b1.value, b2.value, overflow.value

    # iteration body -----------------------------------------------------------
    def field_tensor(self, field):
        """Zero-copy torch view of a state field ([ncell] doubles on the
        engine's device) - for collectives on the engine's memory."""
        import torch
        ptr = self.field_device_pointer(field)
        n = self.n

        class _View:
            __cuda_array_interface__ = {
                "shape": (n,), "typestr": "<f8", "data": (int(ptr), False),
                "version": 2}
        return torch.as_tensor(_View(), device="cuda")

    def refresh_transport_records(self):
        self._check(self._lib.cmi_gpu_refresh_transport_records(self._h))

    def reset_grid(self):
        self._check(self._lib.cmi_gpu_reset_grid(self._h))

    def shoot(self, seed, iteration, first_packet, n_packets):
        self._check(self._lib.cmi_gpu_shoot(self._h, seed, iteration,
                                            first_packet, n_packets))

    def get_counters(self):
        tw = C.c_double()
        tc = np.zeros(NTYPE)
        ns = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_counters(self._h, C.byref(tw),
                                                   _p(tc), C.byref(ns)))
        return tw.value, tc, ns.value

    def get_atomic_count(self):
        n = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_atomic_count(self._h, C.byref(n)))
        return n.value

    def get_phase_clocks(self):
        """Experiment builds with set_tuning(phase_stamps=1): the stamps of
        the last first-generation launch - (cycles per section [5], the
        100 MHz clock at the launch's start, ... at every block's end)."""
        n = C.c_int64()
        self._check(self._lib.cmi_gpu_get_phase_clocks(self._h, None, 0,
                                                       C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        self._check(self._lib.cmi_gpu_get_phase_clocks(
            self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value,
            C.byref(n)))
        return out[:5], int(out[5]), out[6:]

    def get_launch_times(self):
        """[(ms, flights)] of the transport launches since the last
        get_timing(reset=True)."""
        n = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_launch_times(self._h, 0, None, None,
                                                       C.byref(n)))
        ms = np.zeros(max(n.value, 1))
        pk = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._check(self._lib.cmi_gpu_get_launch_times(
            self._h, n.value, _p(ms),
            pk.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))
        return list(zip(ms[:n.value].tolist(), pk[:n.value].tolist()))

    def get_launch_steps(self):
        """The DDA step counter (steps since the last reset_grid) after each
        transport launch since the last get_timing(reset=True)."""
        n = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_launch_steps(self._h, 0, None,
                                                       C.byref(n)))
        st = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._check(self._lib.cmi_gpu_get_launch_steps(
            self._h, n.value, st.ctypes.data_as(C.POINTER(C.c_uint64)),
            C.byref(n)))
        return st[:n.value].tolist()

    # decomposed grids ---------------------------------------------------------
    def set_export_buffer(self, device_pointer, capacity):
        self._check(self._lib.cmi_gpu_set_export_buffer(
            self._h, device_pointer, int(capacity)))

    def get_export_count(self):
        n = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_export_count(self._h, C.byref(n)))
        return n.value

    def reset_exports(self):
        self._check(self._lib.cmi_gpu_reset_exports(self._h))

    def shoot_flights(self, seed, iteration, first_packet, device_pointer, n):
        self._check(self._lib.cmi_gpu_shoot_flights(
            self._h, seed, iteration, int(first_packet), device_pointer,
            int(n)))

    def get_wave_steps(self):
        n = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_wave_steps(self._h, C.byref(n)))
        return n.value

    def update_cells(self, loop, totweight):
        self._check(self._lib.cmi_gpu_update_cells(self._h, loop, totweight))

    def update_cells_range(self, loop, totweight, first_cell, ncell):
        self._check(self._lib.cmi_gpu_update_cells_range(
            self._h, loop, totweight, first_cell, ncell))

    def compute_emissivities(self, lines=None, first_cell=0, ncell=None):
        """EmissivityCalculator::calculate_emissivities
        (src/EmissivityCalculator.cpp:439-470) for the cells [first_cell,
        first_cell + ncell): {line name: array over those cells}. `lines` are
        names from EMISSION_LINES (all of them by default)."""
        names = list(EMISSION_LINES if lines is None else lines)
        idx = _line_indices(names)
        if ncell is None:
            ncell = self.n - first_cell
        out = np.empty((len(names), ncell))
        self._check(self._lib.cmi_gpu_compute_emissivities(
            self._h, len(names), idx,
            first_cell, ncell, out.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(names, out))

    def set_spectrum_trackers(self, positions, nbins=100, opening_angles=None,
                              reference_directions=None):
        """SpectrumTrackers in the cells that hold `positions` ([n][3])."""
        pos = _f64(positions).reshape(-1, 3)
        n = len(pos)
        ang = None if opening_angles is None else _f64(opening_angles)
        ref = None if reference_directions is None else \
            _f64(reference_directions).reshape(-1, 3)
        self._check(self._lib.cmi_gpu_set_spectrum_trackers(
            self._h, n, _p(pos) if n else None, nbins,
            None if ang is None else _p(ang),
            None if ref is None else _p(ref)))
        self._trackers = (n, nbins)

    def set_trackers(self, positions, kinds, nbins=100, opening_angles=None,
                     reference_directions=None):
        """Trackers of the given kinds (TRACKER_SPECTRUM / TRACKER_ABSORPTION)
        in the cells that hold `positions` ([n][3]); nbins: one number for
        all, or one per tracker."""
        pos = _f64(positions).reshape(-1, 3)
        n = len(pos)
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        assert kinds.size == n
        bins = np.ascontiguousarray(
            np.broadcast_to(np.asarray(nbins, dtype=np.int32), (n,)))
        ang = None if opening_angles is None else _f64(opening_angles)
        ref = None if reference_directions is None else \
            _f64(reference_directions).reshape(-1, 3)
        self._check(self._lib.cmi_gpu_set_trackers(
            self._h, n, _p(pos) if n else None,
            kinds.ctypes.data_as(C.POINTER(C.c_int32)),
            bins.ctypes.data_as(C.POINTER(C.c_int32)),
            None if ang is None else _p(ang),
            None if ref is None else _p(ref)))
        self._trackers = (n, bins.tolist())

    def get_tracker_absorption(self):
        """absorption[tracker][photon type (4)][ion (14)]: the sums of an
        AbsorptionTracker (zero rows for spectrum trackers)"""
        n, _ = self._trackers
        out = np.zeros((n, 4, NION))
        self._check(self._lib.cmi_gpu_get_tracker_absorption(self._h, _p(out)))
        return out

    def set_tracker_frequency_bins(self, tracker, kind="Linear",
                                   minimum_frequency=0., maximum_frequency=0.):
        """FrequencyBins of a weighted spectrum tracker: "Linear" between
        the two frequencies (Hz) or "Level" (one bin per ion)."""
        self._check(self._lib.cmi_gpu_set_tracker_frequency_bins(
            self._h, tracker, {"Linear": 0, "Level": 1}[kind],
            minimum_frequency, maximum_frequency))

    def get_tracker_flux(self):
        """flux[tracker][photon type (4)][bin]: the sums of the weighted
        spectrum trackers (zeros for the other kinds); a list of [4][bins]
        arrays"""
        n, nbins = self._trackers
        bins = [nbins] * n if np.isscalar(nbins) else list(nbins)
        flat = np.zeros(4 * max(sum(bins), 1))
        self._check(self._lib.cmi_gpu_get_tracker_flux(self._h, _p(flat)))
        out, at = [], 0
        for b in bins:
            out.append(flat[at:at + 4 * b].reshape(4, b))
            at += 4 * b
        return out

    def enable_trackers(self, on=True):
        self._check(self._lib.cmi_gpu_enable_trackers(self._h, int(on)))

    def get_tracker_counts(self):
        """counts[tracker][type (primary, diffuse H, diffuse He)][bin]: one
        array when all trackers have the same number of bins, else a list of
        [3][bins] arrays."""
        n, nbins = self._trackers
        bins = [nbins] * n if np.isscalar(nbins) else list(nbins)
        flat = np.zeros(3 * max(sum(bins), 1), dtype=np.uint64)
        self._check(self._lib.cmi_gpu_get_tracker_counts(
            self._h, flat.ctypes.data_as(C.POINTER(C.c_uint64))))
        out, at = [], 0
        for b in bins:
            out.append(flat[at:at + 3 * b].reshape(3, b))
            at += 3 * b
        if len(set(bins)) <= 1:
            return np.array(out).reshape(n, 3, bins[0] if bins else 0)
        return out

    # escape maps ------------------------------------------------------------
    def set_escape_tally(self, nlon, nmu, frame=IDENTITY_FRAME, nfreq=1,
                         bins="Linear", minimum_frequency=3.289e15,
                         maximum_frequency=4. * 3.289e15):
        """A tally of the packets that leave the whole box, by photon type,
        frequency bin ("Linear": nfreq bins between the two frequencies;
        "Level": the 14 level bins) and the equal-area pixel of their
        direction in `frame` (include/cmi_gpu.h, "escape maps"). Counts while
        trackers are enabled. nlon = 0 removes it."""
        kind = {"Linear": 0, "Level": 1}[bins]
        if kind == 1:
            nfreq = NION
        self._check(self._lib.cmi_gpu_set_escape_tally(
            self._h, int(nlon), int(nmu), _p(_f64(frame).reshape(9)),
            int(nfreq), kind, minimum_frequency, maximum_frequency))
        self._escape = (int(nfreq), int(nlon), int(nmu)) if nlon else None

    def reset_escape_tally(self):
        self._check(self._lib.cmi_gpu_reset_escape_tally(self._h))

    def escape_tally(self):
        """The sums (3, nfreq, nlon, nmu) in packet weight since the tally
        was set or reset."""
        shape = self._escape if self._escape is not None else (1, 1, 1)
        out = np.zeros((3,) + shape)
        self._check(self._lib.cmi_gpu_download_escape_tally(self._h, _p(out)))
        return out

    # SPH mappings -----------------------------------------------------------
    def _sph_arguments(self, positions, h, kernel, periodic_box, grid):
        pos = _f64(positions).reshape(-1, 3)
        hh = _f64(h).reshape(-1)
        if len(hh) != len(pos):
            raise ValueError("%d positions, %d smoothing lengths" %
                             (len(pos), len(hh)))
        anchor, sides, ncell = grid if grid is not None else self._grid
        box = None
        if periodic_box is not None:
            box = _f64(periodic_box).reshape(6)
        nc = (C.c_int32 * 3)(*[int(n) for n in ncell])
        return (pos, hh, SPH_KERNELS[kernel], box, _f64(anchor).reshape(3),
                _f64(sides).reshape(3), nc, tuple(int(n) for n in ncell))

    def _sph_check(self, rc):
        if rc == EDECLINED:
            raise SphMapDeclined(
                self._lib.cmi_gpu_last_error().decode(),
                SPH_DECLINE_REASONS[self.sph_map_stats()["declined"]])
        self._check(rc)

    def sph_map_to_cells(self, positions, h, amplitudes, kernel="spline_h",
                         periodic_box=None, grid=None):
        """out[k][c] = sum_i amplitudes[k][i] W(|c - p_i|, h_i) at the cell
        midpoints c of `grid` = (anchor, sides, ncell), by default the
        engine's whole grid: (K, nx, ny, nz) for K <= 4 amplitude arrays
        (K, n) or one (n,). kernel: "spline_h" (CubicSplineKernel, support h)
        or "spline_2h" (Price 2007, support 2 h). periodic_box: None or
        (anchor[3], sides[3]), minimum image per axis. Raises SphMapDeclined
        when the call declines (include/cmi_gpu.h, "SPH mappings")."""
        pos, hh, form, box, anchor, sides, nc, ncell = self._sph_arguments(
            positions, h, kernel, periodic_box, grid)
        amp = _f64(amplitudes)
        if amp.ndim == 1:
            amp = amp.reshape(1, -1)
        if amp.ndim != 2 or amp.shape[1] != len(hh):
            raise ValueError("amplitudes of shape %r for %d particles" %
                             (amp.shape, len(hh)))
        out = np.zeros((amp.shape[0],) + ncell)
        self._sph_check(self._lib.cmi_gpu_sph_map_to_cells(
            self._h, form, len(hh), _p(pos), _p(hh), amp.shape[0], _p(amp),
            _p_or_none(box), _p(anchor), _p(sides), nc, _p(out)))
        return out

    def sph_map_to_particles(self, positions, h, cell_values,
                             kernel="spline_h", periodic_box=None, grid=None):
        """out[i] = sum_c W(|c - p_i|, h_i) cell_values[c] over the cell
        midpoints of `grid`: (n,). Arguments as sph_map_to_cells."""
        pos, hh, form, box, anchor, sides, nc, ncell = self._sph_arguments(
            positions, h, kernel, periodic_box, grid)
        g = _f64(cell_values).reshape(-1)
        if len(g) != int(np.prod(ncell)):
            raise ValueError("%d cell values for %r cells" % (len(g), ncell))
        out = np.zeros(len(hh))
        self._sph_check(self._lib.cmi_gpu_sph_map_to_particles(
            self._h, form, len(hh), _p(pos), _p(hh), _p_or_none(box),
            _p(anchor), _p(sides), nc, _p(g), _p(out)))
        return out

    def sph_map_stats(self):
        """What the last SPH mapping of this engine did."""
        raw = (C.c_int64 * 8)()
        self._check(self._lib.cmi_gpu_get_sph_map_stats(self._h, raw))
        names = ("tiles", "list_entries", "longest_list", "stage_chunk",
                 "wave_class", "lane_class", "declined", "kernel_ns")
        return {name: int(raw[k]) for k, name in enumerate(names)}

    def cross_sections(self, frequencies):
        """The engine's cross sections (n, 14) in m^2 at frequencies in Hz."""
        nu = _f64(frequencies).reshape(-1)
        out = np.zeros((len(nu), NION))
        self._check(self._lib.cmi_gpu_cross_sections(self._h, len(nu), _p(nu),
                                                     _p(out)))
        return out

    def ionizing_columns(self, origin, directions):
        """Column densities N[ray][ion] (m^-2) of the 14 ions from `origin`
        (m) along the unit vectors directions[nrays][3] to the edge of the
        box, from the state on the device: the hydrogen density times the
        element's abundance times the ionic fraction, through
        render_field_sky (whose surface brightness is the line integral over
        4 pi; like it, not for periodic boxes or blocks of a decomposed
        grid)."""
        n_H = self.download_field(FIELD_NUMBER_DENSITY)
        abundance = {"H": 1.}
        abundance.update(zip(("He", "C", "N", "O", "Ne", "S"),
                             self._abundances))
        fields = np.empty((NION, self.n))
        for ion in range(NION):
            fields[ion] = (n_H * abundance[_ION_ELEMENTS[ion]] *
                           self.download_field(FIELD_IONIC_FRACTION + ion))
        return np.ascontiguousarray(
            4. * np.pi * self.render_field_sky(fields, origin, directions).T)

    def ionizing_optical_depths(self, origin, directions, frequencies):
        """tau[ray][frequency] of the ionizing continuum from `origin` to the
        edge of the box: ionizing_columns @ cross_sections."""
        return (self.ionizing_columns(origin, directions) @
                self.cross_sections(frequencies).T)

    def set_tuning(self, **kw):
        for k, v in kw.items():
            self._check(self._lib.cmi_gpu_set_tuning(self._h, k.encode(),
                                                     int(v)))

    def synchronize(self):
        self._check(self._lib.cmi_gpu_synchronize(self._h))

    # probes -------------------------------------------------------------------
    def emit_packets(self, seed, iteration, first_packet, n):
        pos = np.empty((n, 3))
        dirn = np.empty((n, 3))
        nu = np.empty(n)
        sig = np.empty((n, NION))
        tau = np.empty(n)
        self._check(self._lib.cmi_gpu_emit_packets(
            self._h, seed, iteration, first_packet, n, _p(pos), _p(dirn),
            _p(nu), _p(sig), _p(tau)))
        return pos, dirn, nu, sig, tau

    def order_packets(self, seed, iteration, first_packet, n):
        """(ids, keys) of the order a shoot of these n packets - one launch -
        would fly them in: position j is packet first_packet + ids[j], its
        sort key keys[j]."""
        ids = np.empty(n, dtype=np.uint32)
        keys = np.empty(n, dtype=np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self._check(self._lib.cmi_gpu_order_packets(
            self._h, seed, iteration, first_packet, n,
            ids.ctypes.data_as(u32), keys.ctypes.data_as(u32)))
        return ids, keys

    def trace_packets(self, position, direction, tau, sigma_H, sigma_He_corr,
                      max_steps):
        pos = _f64(position).reshape(-1, 3)
        n = pos.shape[0]
        dirn = _f64(direction).reshape(n, 3)
        tau = _f64(tau).reshape(n)
        sh = _f64(sigma_H).reshape(n)
        she = _f64(sigma_He_corr).reshape(n)
        cells = np.empty((n, max_steps), dtype=np.int64)
        ds = np.empty((n, max_steps))
        nsteps = np.empty(n, dtype=np.int32)
        last = np.empty(n, dtype=np.int64)
        final = np.empty((n, 3))
        self._check(self._lib.cmi_gpu_trace_packets(
            self._h, n, _p(pos), _p(dirn), _p(tau), _p(sh), _p(she), max_steps,
            cells.ctypes.data_as(C.POINTER(C.c_int64)), _p(ds),
            nsteps.ctypes.data_as(C.POINTER(C.c_int32)),
            last.ctypes.data_as(C.POINTER(C.c_int64)), _p(final)))
        return cells, ds, nsteps, last, final

    def sample_spectrum(self, kind, temperature, seed, n):
        out = np.empty(n)
        self._check(self._lib.cmi_gpu_sample_spectrum(
            self._h, kind, temperature, seed, n, _p(out)))
        return out

    def thermal_probe(self, solve, J, heating, temperature, number_density):
        J = _f64(J).reshape(-1, NION)
        n = J.shape[0]
        heating = _f64(heating).reshape(n, 2)
        T = _f64(temperature).reshape(n)
        dens = _f64(number_density).reshape(n)
        x = np.empty((n, NION))
        Tout = np.empty(n)
        pair = np.empty((n, 2))
        self._check(self._lib.cmi_gpu_thermal_probe(
            self._h, n, int(solve), _p(J), _p(heating), _p(T), _p(dens),
            _p(x), _p(Tout), _p(pair)))
        return x, Tout, pair

    def physics_probe(self, kind, rows):
        """Atomic-data functions on the device for the given input rows; kind
        0 cross sections (nu), 1 recombination rates (T), 2 line cooling
        ({T, n_e, 13 abundances}), 3 re-emission probabilities (T), 4 charge
        transfer rates (T4)."""
        width_in = (1, 1, 15, 1, 1)[kind]
        width_out = (14, 14, 1, 5, 42)[kind]
        rows = _f64(rows).reshape(-1, width_in)
        out = np.zeros((rows.shape[0], width_out))
        self._check(self._lib.cmi_gpu_physics_probe(
            self._h, kind, rows.shape[0], _p(rows), _p(out)))
        return out

    # dusty radiative transfer ------------------------------------------------
    def set_dust_scattering(self, g, p_l, albedo, kappa):
        self._check(self._lib.cmi_gpu_set_dust_scattering(
            self._h, g, p_l, albedo, kappa))

    def set_dust_scattering_per_hydrogen(self, g, p_l, albedo, sigma):
        """Dust that follows the gas: opacity n sigma, sigma in m^2 per
        hydrogen nucleus (x_H is not read)."""
        self._check(self._lib.cmi_gpu_set_dust_scattering_per_hydrogen(
            self._h, g, p_l, albedo, sigma))

    def set_cell_source_line(self, line):
        """Packets of dust_shoot / dust_probe start in the cells, in
        proportion to the emissivity of `line` (a name from EMISSION_LINES)
        of the cells as they are."""
        self._check(self._lib.cmi_gpu_set_cell_source_line(
            self._h, EMISSION_LINES.index(line)))

    def set_cell_source_field(self, field):
        """The same for a per-cell luminosity density field[ncell] (W m^-3)
        of the caller's."""
        f = _f64(field).reshape(self.n)
        self._check(self._lib.cmi_gpu_set_cell_source_field(self._h, _p(f)))

    def get_cell_source(self, tables=True):
        """The cell source's total luminosity (W) and, with `tables`, its
        block sums [ceil(ncell / 256)] and cell sums [ncell]."""
        total = C.c_double()
        if not tables:
            self._check(self._lib.cmi_gpu_get_cell_source(
                self._h, C.byref(total), None, None))
            return total.value
        blocks = np.zeros((self.n + 255) // 256)
        cells = np.zeros(self.n)
        self._check(self._lib.cmi_gpu_get_cell_source(
            self._h, C.byref(total), _p(blocks), _p(cells)))
        return total.value, blocks, cells

    def set_ccd_image(self, theta, phi, nx, ny, anchor, sides):
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        self._check(self._lib.cmi_gpu_set_ccd_image(
            self._h, theta, phi, int(nx), int(ny), _p(a), _p(s)))
        self.image_shape = (int(nx), int(ny))
        self.nviews = 1

    def set_ccd_images(self, theta, phi, nx, ny, anchors, sides):
        """Several CCD images filled by one run: view v looks along
        (theta[v], phi[v]) with anchors[v] and sides[v] ((2,) arrays serve
        every view); the resolution is shared (include/cmi_gpu.h,
        cmi_gpu_set_ccd_images). download_images returns the stack."""
        t = _f64(theta).reshape(-1)
        f = _f64(phi).reshape(-1)
        n = len(t)
        if len(f) != n:
            raise ValueError("theta and phi differ in length")
        a = _f64(np.broadcast_to(_f64(anchors), (n, 2)))
        s = _f64(np.broadcast_to(_f64(sides), (n, 2)))
        self._check(self._lib.cmi_gpu_set_ccd_images(
            self._h, n, _p(t), _p(f), int(nx), int(ny), _p(a), _p(s)))
        self.image_shape = (int(nx), int(ny))
        self.nviews = n

    def download_images(self):
        """The images of every view, (nviews, 3, nx, ny), unnormalised"""
        out = np.zeros((self.nviews, 3) + self.image_shape)
        for v in range(self.nviews):
            out[v] = self.download_image_view(v)
        return out

    def download_image_view(self, view):
        """I, Q, U of one view, (3, nx, ny), unnormalised"""
        out = np.zeros((3,) + self.image_shape)
        self._check(self._lib.cmi_gpu_download_image_view(
            self._h, int(view), _p(out[0]), _p(out[1]), _p(out[2])))
        return out

    def get_dust_view_counters(self, view):
        """One view's share of a run with several views: the DDA steps of its
        own marches, the atomics into its image, its events inside the
        exclusion radius and outside the window"""
        c = (C.c_uint64 * 4)()
        self._check(self._lib.cmi_gpu_get_dust_view_counters(
            self._h, int(view), c))
        return dict(zip(("nsteps", "natomics", "nexcluded", "noutside"),
                        (int(v) for v in c)))

    def select_probe_view(self, view):
        """The view that the TRACE and SKY_PEEL probes follow (0 after a
        camera is set)"""
        self._check(self._lib.cmi_gpu_select_probe_view(self._h, int(view)))

    def set_continuous_source_spiral_galaxy(self, r_stars, h_stars,
                                            bulge_over_total):
        self._check(self._lib.cmi_gpu_set_continuous_source_spiral_galaxy(
            self._h, r_stars, h_stars, bulge_over_total))

    def dust_shoot(self, seed, first_packet, n):
        self._check(self._lib.cmi_gpu_dust_shoot(self._h, seed, first_packet,
                                                 n))

    def download_image(self):
        """I, Q, U as an array of shape (3, nx, ny), unnormalised"""
        out = np.zeros((3,) + self.image_shape)
        self._check(self._lib.cmi_gpu_download_image(
            self._h, _p(out[0]), _p(out[1]), _p(out[2])))
        return out

    def reset_image(self):
        self._check(self._lib.cmi_gpu_reset_image(self._h))

    def get_dust_counters(self):
        c = (C.c_uint64 * 6)()
        self._check(self._lib.cmi_gpu_get_dust_counters(self._h, c))
        return dict(zip(("nsteps", "nscatter", "ncapped", "natomics",
                         "npackets", "nsource_capped"), (int(v) for v in c)))

    def dust_probe(self, kind, seed, first_packet, n, rows=None,
                   max_events=0):
        """Device dust functions, one row per packet (include/cmi_gpu.h,
        cmi_gpu_dust_probe); returns the output rows."""
        width = {DUST_PROBE_EMIT: 6, DUST_PROBE_SCATTER: 12,
                 DUST_PROBE_SCATTER_TOWARDS: 5,
                 DUST_PROBE_OPTICAL_DEPTH: 2 + max_events,
                 DUST_PROBE_TRACE: 4 + 8 * max_events,
                 DUST_PROBE_CELL_SOURCE: 7, DUST_PROBE_SKY_PEEL: 9,
                 DUST_PROBE_CUBE_TRACE: 4 + 10 * max_events}[kind]
        in_width = {DUST_PROBE_SCATTER: 12, DUST_PROBE_SCATTER_TOWARDS: 12,
                    DUST_PROBE_OPTICAL_DEPTH: 6,
                    DUST_PROBE_SKY_PEEL: 15}.get(kind, 0)
        inp = None
        if in_width:
            inp = _f64(rows).reshape(n, in_width)
        out = np.zeros((n, width))
        self._check(self._lib.cmi_gpu_dust_probe(
            self._h, kind, seed, first_packet, n,
            _p_or_none(inp), _p(out), max_events))
        return out

    # emission-line images ----------------------------------------------------
    def render_line_images(self, lines, theta, phi, nx, ny, anchor, sides,
                           supersample=1, dust_cross_section=0.):
        """Line-of-sight maps of emission lines (names from EMISSION_LINES;
        None: all) for the view (theta, phi): {name: (nx, ny) array} in
        W m^-2 sr^-1, dust of `dust_cross_section` m^2 per hydrogen nucleus
        along the way (include/cmi_gpu.h, cmi_gpu_render_line_images)."""
        names = list(EMISSION_LINES if lines is None else lines)
        idx = _line_indices(names)
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((len(names), max(int(nx), 0), max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_line_images(
            self._h, len(names), idx,
            theta, phi, int(nx), int(ny), _p(a), _p(s), int(supersample),
            dust_cross_section, _p(out)))
        return dict(zip(names, out))

    def render_scattered_line_images(self, lines, theta, phi, nx, ny, anchor,
                                     sides, npackets, seed, sigma, albedo, g,
                                     p_l):
        """Monte Carlo images of emission lines in direct and dust-scattered
        light: (nlines, 3, nx, ny), I, Q and U in W m^-2 sr^-1. Each line is
        one run of `npackets` packets from the cells' emissivities through
        dust of `sigma` m^2 per hydrogen nucleus (albedo, HG asymmetry g,
        peak linear polarisation p_l); the unnormalised image is scaled by
        L_total / (npackets A_pixel), which makes it comparable with
        render_line_images. Replaces the engine's CCD image, dust and dust
        source.
        With sequences of equal length for theta and phi (anchor and sides
        then (2,) for every view or (nviews, 2)) the views share one run per
        line, hence its noise: (nlines, nviews, 3, nx, ny)."""
        names = list(EMISSION_LINES if lines is None else lines)
        self.set_dust_scattering_per_hydrogen(g, p_l, albedo, sigma)
        several, scaled = self._scattered_parallel_cameras(
            theta, phi, nx, ny, anchor, sides, npackets)
        images, _ = self._scattered_line_runs(names, npackets, seed, scaled)
        return images if several else images[:, 0]

    # what the four render_scattered_line_* calls share ----------------------
    def _scattered_parallel_cameras(self, theta, phi, nx, ny, anchor, sides,
                                    npackets):
        """Sets the parallel camera, or the several with sequences for theta
        and phi. Returns `several` and scaled(raw, total): the stack raw
        (nviews, 3, ..., nx, ny) of a run of total luminosity `total` times
        L_total / (npackets A_pixel) of its view."""
        several = bool(np.ndim(theta) or np.ndim(phi))
        nviews = len(_f64(theta).reshape(-1)) if several else 1
        a = _f64(np.broadcast_to(_f64(anchor), (nviews, 2)))
        s = _f64(np.broadcast_to(_f64(sides), (nviews, 2)))
        pixel_area = s[:, 0] * s[:, 1] / (int(nx) * int(ny))
        if several:
            self.set_ccd_images(theta, phi, nx, ny, a, s)
        else:
            self.set_ccd_image(theta, phi, nx, ny, a[0], s[0])

        def scaled(raw, total):
            scale = total / (int(npackets) * pixel_area)
            return raw * scale.reshape((-1,) + (1,) * (raw.ndim - 1))
        return several, scaled

    def _scattered_point_cameras(self, origin, nlon, nlat, exclusion_radius,
                                 lon_range, lat_range, frame_pole,
                                 frame_zero_longitude, direct_light,
                                 npackets):
        """Sets the sky camera, or the several with origin of shape (nviews,
        3): the frames, the cameras, the pixels' solid angles. Returns
        `several`, the number of observers and scaled(raw, total): the stack
        raw (nviews, 3, ..., nlon, nlat) times L_total / (npackets
        omega_ij)."""
        several = np.ndim(origin) == 2
        o = _f64(origin).reshape(-1, 3)
        nviews = len(o)
        poles = np.broadcast_to(_f64(frame_pole), (nviews, 3))
        zeros = np.broadcast_to(_f64(frame_zero_longitude), (nviews, 3))
        frames = np.array([sky_frame(p, z) for p, z in zip(poles, zeros)])
        if several:
            self.set_sky_cameras(o, nlon, nlat, exclusion_radius, lon_range,
                                 lat_range, frames, direct_light)
        else:
            self.set_sky_camera(o[0], nlon, nlat, exclusion_radius, lon_range,
                                lat_range, frames[0], direct_light)
        omega = np.array([
            sky_map_directions(nlon, nlat, lon_range, lat_range, f)[1]
            for f in frames])

        def scaled(raw, total):
            return raw * (total / int(npackets)) / omega.reshape(
                (nviews,) + (1,) * (raw.ndim - 3) + (int(nlon), int(nlat)))
        return several, nviews, scaled

    def _scattered_line_runs(self, names, npackets, seed, scaled, cube=None):
        """One run of npackets packets per line into the cameras as set: the
        scaled images (nlines, nviews, 3, nx, ny) and, with cube = (nchan,
        vmin, vmax, sigma_turb, observer_velocities), the scaled cubes
        (nlines, nviews, 3, nchan, nx, ny) of cube mode, which is set anew
        for every line and left off."""
        shape = (len(names), self.nviews, 3)
        images = np.zeros(shape + self.image_shape)
        cubes = None if cube is None else \
            np.zeros(shape + (int(cube[0]),) + self.image_shape)
        try:
            for k, name in enumerate(names):
                self.set_cell_source_line(name)
                if cube is None:
                    self.reset_image()
                else:
                    self.set_scattered_cube(*cube[:4],
                                            observer_velocities=cube[4])
                self.dust_shoot(seed, 0, int(npackets))
                total = self.get_cell_source(tables=False)
                images[k] = scaled(self.download_images(), total)
                if cube is not None:
                    cubes[k] = scaled(self.download_cubes(), total)
        finally:
            if cube is not None:
                self.set_scattered_cube(0, 0., 1.)
        return images, cubes

    def render_field_images(self, fields, theta, phi, nx, ny, anchor, sides,
                            supersample=1, extinction=None):
        """The same maps of any per-cell quantities: fields[nfields][ncell]
        and the optional extinction[ncell] (m^-1); (nfields, nx, ny)."""
        f = _f64(fields).reshape(-1, self.n)
        k = None if extinction is None else _f64(extinction).reshape(self.n)
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((len(f), max(int(nx), 0), max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_field_images(
            self._h, len(f), _p(f), theta, phi, int(nx), int(ny), _p(a),
            _p(s), int(supersample), _p_or_none(k),
            _p(out)))
        return out

    def line_image_probe(self, theta, phi, xy, max_cells):
        """The rays through the image coordinates xy[n][2]: rows {t_in, t_out,
        steps, cells[max_cells], ds[max_cells]}."""
        xy = _f64(xy).reshape(-1, 2)
        out = np.zeros((len(xy), 3 + 2 * max_cells))
        self._check(self._lib.cmi_gpu_line_image_probe(
            self._h, theta, phi, len(xy), _p(xy), max_cells, _p(out)))
        return out

    # spectral line cubes ----------------------------------------------------
    def set_cell_velocities(self, velocities):
        """The cells' bulk velocities for render_line_cube: (3, ncell) in
        m s^-1, in the engine's cell order; None puts every cell at rest."""
        if velocities is None:
            self._check(self._lib.cmi_gpu_set_cell_velocities(self._h, None))
            return
        v = _f64(velocities).reshape(3, self.n)
        self._check(self._lib.cmi_gpu_set_cell_velocities(self._h, _p(v)))

    def render_line_cube(self, lines, theta, phi, nx, ny, anchor, sides,
                         nchan, vmin, vmax, supersample=1,
                         dust_cross_section=0., sigma_turb=0.):
        """render_line_images resolved in radial velocity: {name: (nchan, nx,
        ny) array}, W m^-2 sr^-1 per channel, for `nchan` channels of equal
        width over [vmin, vmax) m s^-1 (positive: receding). Each cell's
        emission is shifted by its velocity (set_cell_velocities) along the
        view and spread by the thermal width of the emitting ion plus
        `sigma_turb` (include/cmi_gpu.h, cmi_gpu_render_line_cube). Only
        names of LINE_ATOMIC_WEIGHTS have a cube."""
        names = list(lines)
        idx = _line_indices(names)
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((len(names), max(int(nchan), 0), max(int(nx), 0),
                        max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_line_cube(
            self._h, len(names), idx,
            theta, phi, int(nx), int(ny), _p(a), _p(s), int(supersample),
            dust_cross_section, int(nchan), vmin, vmax, sigma_turb, _p(out)))
        return dict(zip(names, out))

    def render_field_cube(self, fields, widths, theta, phi, nx, ny, anchor,
                          sides, nchan, vmin, vmax, supersample=1,
                          extinction=None, velocity=None):
        """The same cubes of any per-cell sources: fields[nfields][ncell]
        with the Gaussian widths[nfields][ncell] (b = sqrt(2) sigma, m s^-1),
        the optional extinction[ncell] (m^-1) and velocity[3][ncell]
        (m s^-1); (nfields, nchan, nx, ny)."""
        f = _f64(fields).reshape(-1, self.n)
        w = _f64(widths).reshape(len(f), self.n)
        k = None if extinction is None else _f64(extinction).reshape(self.n)
        v = None if velocity is None else _f64(velocity).reshape(3, self.n)
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((len(f), max(int(nchan), 0), max(int(nx), 0),
                        max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_field_cube(
            self._h, len(f), _p(f), _p_or_none(k),
            _p_or_none(v), _p(w), theta, phi, int(nx),
            int(ny), _p(a), _p(s), int(supersample), int(nchan), vmin, vmax,
            _p(out)))
        return out

    # sky maps ---------------------------------------------------------------
    def render_line_sky(self, lines, origin, directions,
                        dust_cross_section=0.):
        """Surface brightness of emission lines (names from EMISSION_LINES;
        None: all) seen from `origin` (m) along the unit vectors
        directions[nrays][3]: {name: (nrays,) array} in W m^-2 sr^-1, dust of
        `dust_cross_section` m^2 per hydrogen nucleus along the way
        (include/cmi_gpu.h, cmi_gpu_render_line_sky)."""
        names = list(EMISSION_LINES if lines is None else lines)
        idx = _line_indices(names)
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((len(names), len(d)))
        self._check(self._lib.cmi_gpu_render_line_sky(
            self._h, len(names), idx,
            _p(o), len(d), _p(d), dust_cross_section, _p(out)))
        return dict(zip(names, out))

    def render_field_sky(self, fields, origin, directions, extinction=None):
        """The same of any per-cell quantities: fields[nfields][ncell] and
        the optional extinction[ncell] (m^-1); (nfields, nrays)."""
        f = _f64(fields).reshape(-1, self.n)
        k = None if extinction is None else _f64(extinction).reshape(self.n)
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((len(f), len(d)))
        self._check(self._lib.cmi_gpu_render_field_sky(
            self._h, len(f), _p(f), _p(o), len(d), _p(d),
            _p_or_none(k), _p(out)))
        return out

    def sky_probe(self, origin, directions, max_cells):
        """The rays from `origin` along directions[n][3]: rows {t_start,
        t_out, steps, cells[max_cells], ds[max_cells]}."""
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((len(d), 3 + 2 * max_cells))
        self._check(self._lib.cmi_gpu_sky_probe(
            self._h, _p(o), len(d), _p(d), max_cells, _p(out)))
        return out

    def render_line_sky_map(self, lines, origin, nlon, nlat,
                            lon_range=FULL_SKY_LONGITUDE,
                            lat_range=FULL_SKY_LATITUDE,
                            frame=IDENTITY_FRAME, dust_cross_section=0.):
        """Equirectangular maps of emission lines around `origin`: {name:
        (nlon, nlat) array}, the pixels of sky_map_directions."""
        names = list(EMISSION_LINES if lines is None else lines)
        idx = _line_indices(names)
        o = _f64(origin).reshape(3)
        f = _f64(frame).reshape(9)
        out = np.zeros((len(names), max(int(nlon), 0), max(int(nlat), 0)))
        self._check(self._lib.cmi_gpu_render_line_sky_map(
            self._h, len(names), idx,
            _p(o), _p(f), lon_range[0], lon_range[1], lat_range[0],
            lat_range[1], int(nlon), int(nlat), dust_cross_section, _p(out)))
        return dict(zip(names, out))

    # continuum images ---------------------------------------------------------
    def _background(self, background, nf):
        if background is None:
            return None
        return _f64(np.broadcast_to(_f64(background), (nf,)))

    def free_free_coefficients(self, freq):
        """The thermal free-free absorption coefficient (m^-1) and source
        function B_nu(T) (W m^-2 Hz^-1 sr^-1) of the cells as they are at the
        frequencies freq[nf] (Hz): two (nf, ncell) arrays in the engine's
        cell order (include/cmi_gpu.h, "continuum images")."""
        nu = _f64(freq).reshape(-1)
        kappa = np.zeros((len(nu), self.n))
        source = np.zeros((len(nu), self.n))
        self._check(self._lib.cmi_gpu_free_free_coefficients(
            self._h, len(nu), _p(nu), _p(kappa), _p(source)))
        return kappa, source

    def render_continuum_images(self, freq, theta, phi, nx, ny, anchor, sides,
                                supersample=1, background=None):
        """Radio continuum images of the ionized gas for the view (theta,
        phi): (nf, nx, ny), the specific intensity in W m^-2 Hz^-1 sr^-1 at
        freq[nf] (Hz), free-free emission with its own absorption along the
        ray, in front of `background` (a scalar or [nf]; None: nothing). The
        view arguments are those of render_line_images."""
        nu = _f64(freq).reshape(-1)
        bg = self._background(background, len(nu))
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((len(nu), max(int(nx), 0), max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_continuum_images(
            self._h, len(nu), _p(nu), _p_or_none(bg),
            theta, phi, int(nx), int(ny), _p(a), _p(s), int(supersample),
            _p(out)))
        return out

    def render_field_continuum_images(self, kappa, source, theta, phi, nx, ny,
                                      anchor, sides, supersample=1,
                                      background=None):
        """The same images of any channels: kappa[nf][ncell] (m^-1) and
        source[nf][ncell], the per-cell absorption coefficient and source
        function of each channel; (nf, nx, ny)."""
        k = _f64(kappa).reshape(-1, self.n)
        S = _f64(source).reshape(len(k), self.n)
        bg = self._background(background, len(k))
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((len(k), max(int(nx), 0), max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_field_continuum_images(
            self._h, len(k), _p(k), _p(S),
            _p_or_none(bg), theta, phi, int(nx), int(ny),
            _p(a), _p(s), int(supersample), _p(out)))
        return out

    def render_continuum_sky(self, freq, origin, directions, background=None):
        """The free-free continuum seen from `origin` (m) along the unit
        vectors directions[nrays][3]: (nf, nrays) in W m^-2 Hz^-1 sr^-1."""
        nu = _f64(freq).reshape(-1)
        bg = self._background(background, len(nu))
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((len(nu), len(d)))
        self._check(self._lib.cmi_gpu_render_continuum_sky(
            self._h, len(nu), _p(nu), _p_or_none(bg),
            _p(o), len(d), _p(d), _p(out)))
        return out

    def render_field_continuum_sky(self, kappa, source, origin, directions,
                                   background=None):
        """The same of any channels kappa[nf][ncell], source[nf][ncell];
        (nf, nrays)."""
        k = _f64(kappa).reshape(-1, self.n)
        S = _f64(source).reshape(len(k), self.n)
        bg = self._background(background, len(k))
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((len(k), len(d)))
        self._check(self._lib.cmi_gpu_render_field_continuum_sky(
            self._h, len(k), _p(k), _p(S),
            _p_or_none(bg), _p(o), len(d), _p(d),
            _p(out)))
        return out

    def render_continuum_sky_map(self, freq, origin, nlon, nlat,
                                 lon_range=FULL_SKY_LONGITUDE,
                                 lat_range=FULL_SKY_LATITUDE,
                                 frame=IDENTITY_FRAME, background=None):
        """Equirectangular free-free maps around `origin`: (nf, nlon, nlat),
        the pixels of sky_map_directions."""
        nu = _f64(freq).reshape(-1)
        bg = self._background(background, len(nu))
        o = _f64(origin).reshape(3)
        f = _f64(frame).reshape(9)
        lon = _f64(lon_range).reshape(2)
        lat = _f64(lat_range).reshape(2)
        out = np.zeros((len(nu), max(int(nlon), 0), max(int(nlat), 0)))
        self._check(self._lib.cmi_gpu_render_continuum_sky_map(
            self._h, len(nu), _p(nu), _p_or_none(bg),
            _p(o), int(nlon), int(nlat), _p(lon), _p(lat), _p(f), _p(out)))
        return out

    def continuum_probe(self, kappa, source, rays, max_cells, theta=None,
                        phi=None, origin=None, background=None):
        """The march of chosen rays through kappa[nf][ncell] and
        source[nf][ncell], cell by cell: rows {t0, t1, steps,
        cells[max_cells], ds[max_cells], I[nf][max_cells], I_end[nf]}. With
        theta and phi the rays are image coordinates [n][2] of the parallel
        camera, with origin directions [n][3]."""
        k = _f64(kappa).reshape(-1, self.n)
        S = _f64(source).reshape(len(k), self.n)
        nf = len(k)
        bg = self._background(background, nf)
        point = origin is not None
        view = _f64(origin).reshape(3) if point else _f64([theta, phi])
        r = _f64(rays).reshape(-1, 3 if point else 2)
        out = np.zeros((len(r), 3 + (2 + nf) * max_cells + nf))
        self._check(self._lib.cmi_gpu_continuum_probe(
            self._h, nf, _p(k), _p(S), _p_or_none(bg),
            int(point), _p(view), len(r), _p(r), int(max_cells), _p(out)))
        return out

    # absorbing line cubes ---------------------------------------------------
    def _spin(self, spin_temperature):
        """(mode, array or None) of a spin temperature: None (the kinetic
        temperature), one value or one per cell"""
        if spin_temperature is None:
            return HI_SPIN_KINETIC, None
        t = _f64(spin_temperature)
        if t.ndim == 0 or t.size == 1 and self.n != 1:
            return HI_SPIN_FIXED, t.reshape(1)
        return HI_SPIN_CELLS, t.reshape(self.n)

    def _absorbing_fields(self, a, sl, b, velocity, kc, sc):
        return [_f64(a).reshape(self.n), _f64(sl).reshape(self.n),
                _f64(b).reshape(self.n),
                None if velocity is None else _f64(velocity).reshape(3,
                                                                     self.n),
                None if kc is None else _f64(kc).reshape(self.n),
                None if sc is None else _f64(sc).reshape(self.n)]

    def hi_coefficients(self, sigma_turb=0., spin_temperature=None,
                        free_free=True):
        """What the H I calls march, per cell in the engine's cell order: the
        dict {a, sl, b, kc, sc} of the integrated 21-cm opacity (m^-1 m s^-1),
        the line source function B_nu(T_s), the Gaussian width (m s^-1) and
        the free-free absorption coefficient and source function at the line
        (include/cmi_gpu.h, "absorbing line cubes")."""
        mode, ts = self._spin(spin_temperature)
        out = [np.zeros(self.n) for _ in range(5)]
        self._check(self._lib.cmi_gpu_hi_coefficients(
            self._h, sigma_turb, mode, _p_or_none(ts), int(bool(free_free)),
            *[_p(o) for o in out]))
        return dict(zip(("a", "sl", "b", "kc", "sc"), out))

    def render_hi_cube(self, theta, phi, nx, ny, anchor, sides, nchan, vmin,
                       vmax, supersample=1, sigma_turb=0.,
                       spin_temperature=None, free_free=True,
                       background_temperature=0.):
        """The 21-cm cube of the neutral gas for the view (theta, phi):
        (nchan, nx, ny), the specific intensity in W m^-2 Hz^-1 sr^-1 of
        `nchan` channels of equal width over [vmin, vmax) m s^-1, with the
        line's own absorption, the free-free continuum of the ionized gas
        (`free_free`) and a background of `background_temperature` K behind
        the box. `spin_temperature`: None (the cells' kinetic temperature),
        one value or one per cell (K). Velocities from set_cell_velocities;
        the view arguments are those of render_line_images."""
        mode, ts = self._spin(spin_temperature)
        a = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((max(int(nchan), 0), max(int(nx), 0), max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_hi_cube(
            self._h, theta, phi, int(nx), int(ny), _p(a), _p(s),
            int(supersample), int(nchan), vmin, vmax, sigma_turb, mode,
            _p_or_none(ts), int(bool(free_free)), background_temperature,
            _p(out)))
        return out

    def render_hi_sky_cube(self, origin, directions, nchan, vmin, vmax,
                           sigma_turb=0., spin_temperature=None,
                           free_free=True, background_temperature=0.,
                           observer_velocity=None):
        """The 21-cm spectrum along each of the unit vectors
        directions[nrays][3] from `origin` (m): (nchan, nrays). A cell seen
        along d by an observer of `observer_velocity` (m s^-1; None: at rest)
        has the radial velocity (v - v_obs) . d."""
        mode, ts = self._spin(spin_temperature)
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((max(int(nchan), 0), len(d)))
        self._check(self._lib.cmi_gpu_render_hi_sky_cube(
            self._h, _p(o), _p_or_none(vo), len(d), _p(d), int(nchan), vmin,
            vmax, sigma_turb, mode, _p_or_none(ts), int(bool(free_free)),
            background_temperature, _p(out)))
        return out

    def render_hi_sky_map_cube(self, origin, nlon, nlat, nchan, vmin, vmax,
                               lon_range=FULL_SKY_LONGITUDE,
                               lat_range=FULL_SKY_LATITUDE,
                               frame=IDENTITY_FRAME, sigma_turb=0.,
                               spin_temperature=None, free_free=True,
                               background_temperature=0.,
                               observer_velocity=None):
        """The longitude-latitude-velocity cube of the 21-cm line around
        `origin`: (nchan, nlon, nlat), the pixels of sky_map_directions."""
        mode, ts = self._spin(spin_temperature)
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o = _f64(origin).reshape(3)
        f = _f64(frame).reshape(9)
        out = np.zeros((max(int(nchan), 0), max(int(nlon), 0),
                        max(int(nlat), 0)))
        self._check(self._lib.cmi_gpu_render_hi_sky_map_cube(
            self._h, _p(o), _p(f), lon_range[0], lon_range[1], lat_range[0],
            lat_range[1], int(nlon), int(nlat), _p_or_none(vo), int(nchan),
            vmin, vmax, sigma_turb, mode, _p_or_none(ts),
            int(bool(free_free)), background_temperature, _p(out)))
        return out

    def render_field_absorbing_cube(self, a, sl, b, theta, phi, nx, ny, anchor,
                                    sides, nchan, vmin, vmax, supersample=1,
                                    velocity=None, kc=None, sc=None,
                                    background=None):
        """The cube of any absorbing line: a[ncell] the line opacity
        integrated over velocity (m^-1 m s^-1), sl[ncell] its source function,
        b[ncell] the Gaussian widths (m s^-1), optional velocity[3][ncell],
        an optional continuum kc[ncell] (m^-1) and sc[ncell] in the same cells
        and `background` (a scalar or [nchan]); (nchan, nx, ny)."""
        f = self._absorbing_fields(a, sl, b, velocity, kc, sc)
        bg = self._background(background, max(int(nchan), 0))
        an = _f64(anchor).reshape(2)
        s = _f64(sides).reshape(2)
        out = np.zeros((max(int(nchan), 0), max(int(nx), 0), max(int(ny), 0)))
        self._check(self._lib.cmi_gpu_render_field_absorbing_cube(
            self._h, *[_p_or_none(x) for x in f], _p_or_none(bg), theta, phi,
            int(nx), int(ny), _p(an), _p(s), int(supersample), int(nchan),
            vmin, vmax, _p(out)))
        return out

    def render_field_absorbing_sky_cube(self, a, sl, b, origin, directions,
                                        nchan, vmin, vmax, velocity=None,
                                        kc=None, sc=None, background=None,
                                        observer_velocity=None):
        """The same along rays from a point; (nchan, nrays)."""
        f = self._absorbing_fields(a, sl, b, velocity, kc, sc)
        bg = self._background(background, max(int(nchan), 0))
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((max(int(nchan), 0), len(d)))
        self._check(self._lib.cmi_gpu_render_field_absorbing_sky_cube(
            self._h, *[_p_or_none(x) for x in f], _p_or_none(bg), _p(o),
            _p_or_none(vo), len(d), _p(d), int(nchan), vmin, vmax, _p(out)))
        return out

    def absorbing_cube_probe(self, a, sl, b, rays, max_cells, nchan, vmin,
                             vmax, theta=None, phi=None, origin=None,
                             velocity=None, kc=None, sc=None, background=None,
                             observer_velocity=None):
        """The march of chosen rays through the caller's fields, cell by
        cell: rows {t0, t1, steps, cells[max_cells], ds[max_cells],
        I[nchan][max_cells], I_end[nchan]}. With theta and phi the rays are
        image coordinates [n][2] of the parallel camera, with origin
        directions [n][3]."""
        f = self._absorbing_fields(a, sl, b, velocity, kc, sc)
        nchan = int(nchan)
        bg = self._background(background, max(nchan, 0))
        point = origin is not None
        view = _f64(origin).reshape(3) if point else _f64([theta, phi])
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        r = _f64(rays).reshape(-1, 3 if point else 2)
        out = np.zeros((len(r), 3 + (2 + max(nchan, 0)) * max_cells +
                        max(nchan, 0)))
        self._check(self._lib.cmi_gpu_absorbing_cube_probe(
            self._h, *[_p_or_none(x) for x in f], _p_or_none(bg), nchan, vmin,
            vmax, int(point), _p(view), _p_or_none(vo), len(r), _p(r),
            int(max_cells), _p(out)))
        return out

    # absorption spectra -----------------------------------------------------
    @staticmethod
    def _sightlines(origins, directions, lengths):
        d = _f64(directions).reshape(-1, 3)
        o = _f64(np.broadcast_to(_f64(origins).reshape(-1, 3), d.shape))
        if lengths is None:
            lengths = np.inf
        L = _f64(np.broadcast_to(_f64(lengths).reshape(-1), (len(d),)))
        return o, d, L

    def render_field_absorption_spectra(self, n, b, S, g, origins, directions,
                                        nchan, vmin, vmax, lengths=None,
                                        velocity=None, observer_velocity=None):
        """Optical depths of K lines with Voigt profiles along sightlines
        (include/cmi_gpu.h, "absorption spectra"): n[K][ncell] absorber
        densities (m^-3), b[K][ncell] Doppler widths (m s^-1), S[K] and g[K]
        as absorption_line_constants gives them. Sightline r runs from
        origins[r] (one origin serves all) along the unit vector
        directions[r] for lengths[r] metres (None or inf: to the edge of the
        box). Returns tau (nrays, K, nchan) and the column densities N
        (nrays, K), m^-2."""
        S = _f64(S).reshape(-1)
        g = _f64(g).reshape(len(S))
        nn = _f64(n).reshape(len(S), self.n)
        bb = _f64(b).reshape(len(S), self.n)
        v = None if velocity is None else _f64(velocity).reshape(3, self.n)
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o, d, L = self._sightlines(origins, directions, lengths)
        tau = np.zeros((len(d), len(S), max(int(nchan), 0)))
        N = np.zeros((len(d), len(S)))
        self._check(self._lib.cmi_gpu_render_field_absorption_spectra(
            self._h, len(S), _p(nn), _p(bb), _p(S), _p(g), _p_or_none(v),
            len(d), _p(o), _p(d), _p(L), _p_or_none(vo), int(nchan), vmin,
            vmax, _p(tau), _p(N)))
        return tau, N

    def render_absorption_spectra(self, lines, origins, directions, nchan,
                                  vmin, vmax, lengths=None, sigma_turb=0.,
                                  observer_velocity=None):
        """The same for lines of the engine's own ions, from the cells as
        they are: `lines` holds names of ABSORPTION_LINES or tuples (ion
        index, atomic weight, S, g); n = n_H A_element x_ion and b = sqrt(2 k
        T / (w m_u) + 2 sigma_turb^2) are built on the device."""
        rows = []
        for line in lines:
            if isinstance(line, str):
                ion, w, S, g, _ = absorption_table_lines([line])
                rows.append((ion[0], w[0], S[0], g[0]))
            else:
                rows.append(tuple(line))
        ions = np.array([r[0] for r in rows], dtype=np.int32)
        w = _f64([r[1] for r in rows])
        S = _f64([r[2] for r in rows])
        g = _f64([r[3] for r in rows])
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o, d, L = self._sightlines(origins, directions, lengths)
        tau = np.zeros((len(d), len(rows), max(int(nchan), 0)))
        N = np.zeros((len(d), len(rows)))
        self._check(self._lib.cmi_gpu_render_absorption_spectra(
            self._h, len(rows), ions.ctypes.data_as(C.POINTER(C.c_int32)),
            _p(w), _p(S), _p(g), sigma_turb, len(d), _p(o), _p(d), _p(L),
            _p_or_none(vo), int(nchan), vmin, vmax, _p(tau), _p(N)))
        return tau, N

    def absorption_probe(self, n, b, S, g, origin, direction, max_cells,
                         nchan, vmin, vmax, channels=(), length=np.inf,
                         velocity=None, observer_velocity=None):
        """One sightline through one line, cell by cell: {t0, t1, steps,
        cells[max_cells], ds[max_cells], tau[len(channels)][max_cells],
        tau_end[len(channels)]} for up to 8 channels; no skips."""
        nn = _f64(n).reshape(self.n)
        bb = _f64(b).reshape(self.n)
        v = None if velocity is None else _f64(velocity).reshape(3, self.n)
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        ch = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
        out = np.zeros(3 + (2 + len(ch)) * max_cells + len(ch))
        self._check(self._lib.cmi_gpu_absorption_probe(
            self._h, _p(nn), _p(bb), S, g, _p_or_none(v),
            _p(_f64(origin).reshape(3)), _p(_f64(direction).reshape(3)),
            length, _p_or_none(vo), int(nchan), vmin, vmax, len(ch),
            ch.ctypes.data_as(C.POINTER(C.c_int32)), int(max_cells), _p(out)))
        return out

    # sky cubes --------------------------------------------------------------
    def render_field_sky_cube(self, fields, widths, origin, directions, nchan,
                              vmin, vmax, extinction=None, velocity=None,
                              observer_velocity=None):
        """render_field_sky resolved in radial velocity: (nfields, nchan,
        nrays), W m^-2 sr^-1 per channel, for `nchan` channels of equal width
        over [vmin, vmax) m s^-1. A cell of velocity[3][ncell] seen along the
        ray direction d by an observer of `observer_velocity` (m s^-1; None:
        at rest) has the radial velocity (v - v_obs) . d, positive for matter
        that recedes; widths[nfields][ncell] are the Gaussian b = sqrt(2)
        sigma (include/cmi_gpu.h, "sky cubes")."""
        f = _f64(fields).reshape(-1, self.n)
        w = _f64(widths).reshape(len(f), self.n)
        k = None if extinction is None else _f64(extinction).reshape(self.n)
        v = None if velocity is None else _f64(velocity).reshape(3, self.n)
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((len(f), max(int(nchan), 0), len(d)))
        self._check(self._lib.cmi_gpu_render_field_sky_cube(
            self._h, len(f), _p(f), _p_or_none(k),
            _p_or_none(v), _p(w), _p(o),
            _p_or_none(vo), len(d), _p(d), int(nchan),
            vmin, vmax, _p(out)))
        return out

    def render_line_sky_cube(self, lines, origin, directions, nchan, vmin,
                             vmax, dust_cross_section=0., sigma_turb=0.,
                             observer_velocity=None):
        """render_line_sky resolved in radial velocity, a spectrum per ray:
        {name: (nchan, nrays) array}. Velocities from set_cell_velocities,
        widths from the cells' temperatures and `sigma_turb` as in
        render_line_cube. Only names of LINE_ATOMIC_WEIGHTS have a cube."""
        names = list(lines)
        idx = _line_indices(names)
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o = _f64(origin).reshape(3)
        d = _f64(directions).reshape(-1, 3)
        out = np.zeros((len(names), max(int(nchan), 0), len(d)))
        self._check(self._lib.cmi_gpu_render_line_sky_cube(
            self._h, len(names), idx,
            _p(o), _p_or_none(vo), len(d), _p(d),
            dust_cross_section, int(nchan), vmin, vmax, sigma_turb, _p(out)))
        return dict(zip(names, out))

    def render_line_sky_map_cube(self, lines, origin, nlon, nlat, nchan, vmin,
                                 vmax, lon_range=FULL_SKY_LONGITUDE,
                                 lat_range=FULL_SKY_LATITUDE,
                                 frame=IDENTITY_FRAME, dust_cross_section=0.,
                                 sigma_turb=0., observer_velocity=None):
        """render_line_sky_map per velocity channel: {name: (nchan, nlon,
        nlat) array}, the longitude-latitude-velocity cube of an observer at
        `origin`. cube_moments and cube_channel_centres work on it."""
        names = list(lines)
        idx = _line_indices(names)
        vo = (None if observer_velocity is None
              else _f64(observer_velocity).reshape(3))
        o = _f64(origin).reshape(3)
        f = _f64(frame).reshape(9)
        out = np.zeros((len(names), max(int(nchan), 0), max(int(nlon), 0),
                        max(int(nlat), 0)))
        self._check(self._lib.cmi_gpu_render_line_sky_map_cube(
            self._h, len(names), idx,
            _p(o), _p(f), lon_range[0], lon_range[1], lat_range[0],
            lat_range[1], int(nlon), int(nlat), dust_cross_section,
            _p_or_none(vo), int(nchan), vmin, vmax,
            sigma_turb, _p(out)))
        return dict(zip(names, out))

    def set_sky_camera(self, origin, nlon, nlat, exclusion_radius,
                       lon_range=FULL_SKY_LONGITUDE,
                       lat_range=FULL_SKY_LATITUDE, frame=IDENTITY_FRAME,
                       direct_light=True):
        """The peel-offs of dust_shoot go to an observer at `origin` into an
        (nlon, nlat) map of the sky around it (include/cmi_gpu.h,
        cmi_gpu_set_sky_camera); set_ccd_image selects the parallel camera
        again."""
        o = _f64(origin).reshape(3)
        f = _f64(frame).reshape(9)
        self._check(self._lib.cmi_gpu_set_sky_camera(
            self._h, _p(o), _p(f), lon_range[0], lon_range[1], lat_range[0],
            lat_range[1], int(nlon), int(nlat), exclusion_radius,
            int(bool(direct_light))))
        self.image_shape = (int(nlon), int(nlat))
        self.nviews = 1

    def set_sky_cameras(self, origins, nlon, nlat, exclusion_radii,
                        lon_range=FULL_SKY_LONGITUDE,
                        lat_range=FULL_SKY_LATITUDE, frames=IDENTITY_FRAME,
                        direct_light=True):
        """Several sky cameras filled by one run: observer v at origins[v]
        with frames[v] and exclusion_radii[v] (one frame or one radius serves
        every observer); window and resolution are shared (include/cmi_gpu.h,
        cmi_gpu_set_sky_cameras). download_images returns the stack."""
        o = _f64(origins).reshape(-1, 3)
        n = len(o)
        f = _f64(np.broadcast_to(_f64(frames), (n, 3, 3)))
        r = _f64(np.broadcast_to(_f64(exclusion_radii), (n,)))
        self._check(self._lib.cmi_gpu_set_sky_cameras(
            self._h, n, _p(o), _p(f), lon_range[0], lon_range[1],
            lat_range[0], lat_range[1], int(nlon), int(nlat), _p(r),
            int(bool(direct_light))))
        self.image_shape = (int(nlon), int(nlat))
        self.nviews = n

    def get_sky_camera_counters(self):
        c = (C.c_uint64 * 2)()
        self._check(self._lib.cmi_gpu_get_sky_camera_counters(self._h, c))
        return {"nexcluded": int(c[0]), "noutside": int(c[1])}

    def render_scattered_line_sky_map(self, lines, origin, nlon, nlat,
                                      npackets, seed, dust_cross_section,
                                      albedo, g, p_l, exclusion_radius,
                                      lon_range=FULL_SKY_LONGITUDE,
                                      lat_range=FULL_SKY_LATITUDE,
                                      frame_pole=(0., 0., 1.),
                                      frame_zero_longitude=(1., 0., 0.),
                                      direct_light=True):
        """Monte Carlo sky maps of emission lines in direct and
        dust-scattered light around an observer at `origin`: (nlines, 3,
        nlon, nlat), I, Q and U in W m^-2 sr^-1, the pixels and the unit of
        render_line_sky_map. Each line is one run of `npackets` packets from
        the cells' emissivities through dust of `dust_cross_section` m^2 per
        hydrogen nucleus, peeled off towards the observer with a weight
        1 / r^2 (events nearer than `exclusion_radius` add nothing); the raw
        image is scaled by L_total / (npackets omega_ij), omega_ij the exact
        solid angles of sky_map_directions. At albedo 0 it is the ray-traced
        map; with direct_light=False it is the scattered light alone, to be
        added to the ray-traced map. Replaces the engine's camera, dust and
        dust source.
        With a sequence of observers, origin of shape (nviews, 3)
        (exclusion_radius, frame_pole and frame_zero_longitude then one for
        every observer or one each), the observers share one run per line,
        hence its noise: (nlines, nviews, 3, nlon, nlat)."""
        names = list(EMISSION_LINES if lines is None else lines)
        self.set_dust_scattering_per_hydrogen(g, p_l, albedo,
                                              dust_cross_section)
        several, _, scaled = self._scattered_point_cameras(
            origin, nlon, nlat, exclusion_radius, lon_range, lat_range,
            frame_pole, frame_zero_longitude, direct_light, npackets)
        images, _ = self._scattered_line_runs(names, npackets, seed, scaled)
        return images if several else images[:, 0]

    # scattered-light line cubes ---------------------------------------------
    def set_scattered_cube(self, nchan, vmin, vmax, sigma_turb=0.,
                           widths=None, observer_velocities=None):
        """Cube mode of dust_shoot for the cameras as currently set: every
        event also goes, channel by channel, into a velocity cube per view
        (include/cmi_gpu.h, cmi_gpu_set_scattered_cube). `widths` (ncell,) is
        b per cell for a field source (a line source takes the cells'
        temperatures); `observer_velocities` (nviews, 3) the point cameras'.
        nchan = 0 switches cube mode off."""
        w = None if widths is None else _f64(widths).reshape(self.n)
        vo = None if observer_velocities is None else \
            _f64(observer_velocities).reshape(self.nviews, 3)
        self._check(self._lib.cmi_gpu_set_scattered_cube(
            self._h, int(nchan), vmin, vmax, sigma_turb,
            _p_or_none(w),
            _p_or_none(vo)))
        self.cube_channels = int(nchan)

    def download_cubes(self):
        """The cubes of every view, (nviews, 3, nchan, nx, ny), unnormalised"""
        if not self.cube_channels:
            # the engine's own refusal (cube mode is not set)
            self._check(self._lib.cmi_gpu_download_cube_view(
                self._h, 0, None, None, None))
        out = np.zeros((self.nviews, 3, self.cube_channels) +
                       self.image_shape)
        for v in range(self.nviews):
            self._check(self._lib.cmi_gpu_download_cube_view(
                self._h, v, _p(out[v, 0]), _p(out[v, 1]), _p(out[v, 2])))
        return out

    def render_scattered_line_cube(self, lines, theta, phi, nx, ny, anchor,
                                   sides, npackets, seed, sigma, albedo, g,
                                   p_l, nchan, vmin, vmax, sigma_turb=0.):
        """render_scattered_line_images resolved in radial velocity: the
        images (nlines, 3, nx, ny) and the cubes (nlines, 3, nchan, nx, ny)
        of one run per line, both scaled by L_total / (npackets A_pixel):
        W m^-2 sr^-1, per channel for the cubes, the unit of
        render_line_cube. The profile of scattered light carries the
        velocity of the emitting gas as the dust sees it
        (set_cell_velocities) and widens with sigma_turb per scattering.
        With sequences for theta and phi the views share one run per line:
        (nlines, nviews, 3, nx, ny) and (nlines, nviews, 3, nchan, nx, ny).
        Only names of LINE_ATOMIC_WEIGHTS have a cube. Replaces the engine's
        CCD image, dust and dust source, and leaves cube mode off."""
        names = list(lines)
        self.set_dust_scattering_per_hydrogen(g, p_l, albedo, sigma)
        several, scaled = self._scattered_parallel_cameras(
            theta, phi, nx, ny, anchor, sides, npackets)
        images, cubes = self._scattered_line_runs(
            names, npackets, seed, scaled,
            cube=(nchan, vmin, vmax, sigma_turb, None))
        if several:
            return images, cubes
        return images[:, 0], cubes[:, 0]

    def render_scattered_line_sky_map_cube(
            self, lines, origin, nlon, nlat, npackets, seed,
            dust_cross_section, albedo, g, p_l, exclusion_radius, nchan,
            vmin, vmax, sigma_turb=0., observer_velocity=None,
            lon_range=FULL_SKY_LONGITUDE, lat_range=FULL_SKY_LATITUDE,
            frame_pole=(0., 0., 1.), frame_zero_longitude=(1., 0., 0.),
            direct_light=True):
        """render_scattered_line_sky_map resolved in radial velocity, for
        observers of velocity `observer_velocity` ((3,), or (nviews, 3) with
        several observers; None: at rest): the maps (nlines, 3, nlon, nlat)
        and the cubes (nlines, 3, nchan, nlon, nlat), scaled by L_total /
        (npackets omega_ij): the unit of render_line_sky_map_cube. With
        origin of shape (nviews, 3) both gain an axis after the lines'.
        Replaces the engine's camera, dust and dust source, and leaves cube
        mode off."""
        names = list(lines)
        self.set_dust_scattering_per_hydrogen(g, p_l, albedo,
                                              dust_cross_section)
        several, nviews, scaled = self._scattered_point_cameras(
            origin, nlon, nlat, exclusion_radius, lon_range, lat_range,
            frame_pole, frame_zero_longitude, direct_light, npackets)
        vo = None if observer_velocity is None else \
            _f64(np.broadcast_to(_f64(observer_velocity), (nviews, 3)))
        images, cubes = self._scattered_line_runs(
            names, npackets, seed, scaled,
            cube=(nchan, vmin, vmax, sigma_turb, vo))
        if several:
            return images, cubes
        return images[:, 0], cubes[:, 0]

    # Lyman alpha -------------------------------------------------------------
    def set_lyman_alpha(self, nchan, vmin, vmax, sigma_turb=0., x_crit=0.,
                        max_scatter=LYA_MAX_SCATTER, n_HI=None,
                        temperature=None):
        """Lyman-alpha mode for the parallel camera(s), the cell source, the
        dust and the velocities as currently set (include/cmi_gpu.h, "Lyman
        alpha"): builds the per-cell records and zeroes image and cube.
        `n_HI` and `temperature` (ncell,) replace n_H x_H and T of the cells;
        `x_crit` is the core-skipping frequency. nchan = 0 switches it off."""
        n = None if n_HI is None else _f64(n_HI).reshape(self.n)
        t = None if temperature is None else _f64(temperature).reshape(self.n)
        self._check(self._lib.cmi_gpu_set_lyman_alpha(
            self._h, int(nchan), vmin, vmax, sigma_turb, x_crit,
            int(max_scatter), _p_or_none(n), _p_or_none(t)))
        self.lya_channels = int(nchan)
        self.lya_x_crit = float(x_crit)

    def lya_shoot(self, seed, first_packet, n):
        self._check(self._lib.cmi_gpu_lya_shoot(self._h, seed, first_packet,
                                                n))

    def lya_probe(self, kind, seed=0, first_packet=0, n=None, rows=None,
                  max_events=0):
        """Device functions of the Lyman-alpha path, one row per packet
        (include/cmi_gpu.h, cmi_gpu_lya_probe); returns the output rows."""
        in_width = {LYA_PROBE_VOIGT: 4, LYA_PROBE_OPTICAL_DEPTH: 7,
                    LYA_PROBE_SAMPLER: 2}.get(kind, 0)
        inp = None
        if in_width:
            inp = _f64(rows).reshape(-1, in_width)
            n = len(inp)
        width = 6 + 12 * max_events if kind == LYA_PROBE_TRACE else 2
        out = np.zeros((int(n), width))
        self._check(self._lib.cmi_gpu_lya_probe(
            self._h, kind, seed, first_packet, int(n), _p_or_none(inp),
            _p(out), max_events))
        return out

    def download_lya(self):
        """The images (nviews, nx, ny) and the cubes (nviews, nchan, nx, ny)
        of a Lyman-alpha run, unnormalised"""
        if not self.lya_channels:
            # the engine's own refusal (the mode is not set)
            self._check(self._lib.cmi_gpu_download_lya_view(
                self._h, 0, None, None))
        images = np.zeros((self.nviews,) + self.image_shape)
        cubes = np.zeros((self.nviews, self.lya_channels) + self.image_shape)
        for v in range(self.nviews):
            self._check(self._lib.cmi_gpu_download_lya_view(
                self._h, v, _p(images[v]), _p(cubes[v])))
        return images, cubes

    def reset_lya(self):
        self._check(self._lib.cmi_gpu_reset_lya(self._h))

    def get_lya_counters(self):
        c = (C.c_uint64 * 7)()
        self._check(self._lib.cmi_gpu_get_lya_counters(self._h, c))
        return dict(zip(("nsteps", "nhydrogen", "ndust", "nrejections",
                         "natomics", "ncapped", "npackets"),
                        (int(v) for v in c)))

    def set_lya_field(self, enable=True):
        """Switches the radiation field of the Lyman-alpha mode on (zeroed)
        or off: the per-cell tallies of include/cmi_gpu.h, "Lyman alpha
        radiation field". set_lyman_alpha, called anew, switches it off."""
        self._check(self._lib.cmi_gpu_set_lya_field(self._h,
                                                    int(bool(enable))))

    def download_lya_field(self):
        """The raw tallies of a Lyman-alpha run with the field on: a dict of
        the eight arrays (ncell,) L, S_H, S_d, G_x, G_y, G_z, N_H, N_d"""
        rows = np.zeros((self.n, 8))
        self._check(self._lib.cmi_gpu_download_lya_field(self._h, _p(rows)))
        return {name: np.ascontiguousarray(rows[:, k])
                for k, name in enumerate(LYA_FIELD_COLUMNS)}

    def _lya_scale(self, npackets, total_luminosity):
        if total_luminosity is None:
            total_luminosity = self.get_cell_source(tables=False)
        return float(total_luminosity) / int(npackets)

    def lya_radiation_field(self, npackets, total_luminosity=None):
        """The field of a run of `npackets` packets in physical units, a
        dict: `energy_density` (ncell,) in J m^-3, `scattering_rate` (ncell,)
        per atom in s^-1 (0 where the records have no H I; None if the mode
        skips the core, whose skipped scatterings it would leave out),
        `force` (3, ncell) in N m^-3. `total_luminosity` (W): None takes the
        cell source's."""
        s = self._lya_scale(npackets, total_luminosity)
        f = self.download_lya_field()
        per_volume = s / (LIGHTSPEED * self.cell_volume)
        rate = None
        if not self.lya_x_crit > 0.:
            rate = np.zeros(self.n)
            self._check(self._lib.cmi_gpu_lya_spin_temperature(
                self._h, s, 1., 0, _p(rate), _p(np.zeros(self.n))))
        return {"energy_density": f["L"] * per_volume,
                "scattering_rate": rate,
                "force": np.stack([f["G_x"], f["G_y"], f["G_z"]]) *
                per_volume}

    def lya_spin_temperature(self, npackets, background_temperature,
                             collisions=True, total_luminosity=None):
        """(P_alpha, T_s), (ncell,) each: the Lyman-alpha scattering rate per
        atom (s^-1) of a run of `npackets` packets and the 21-cm spin
        temperature (K) it implies against a background of
        `background_temperature` K, with (`collisions`) or without the
        collisional coupling of the cells (include/cmi_gpu.h,
        cmi_gpu_lya_spin_temperature). T_s goes as it is into
        render_hi_cube(spin_temperature=T_s) and its sky variants. Refused if
        the mode skips the core."""
        s = self._lya_scale(npackets, total_luminosity)
        P = np.zeros(self.n)
        T_s = np.zeros(self.n)
        self._check(self._lib.cmi_gpu_lya_spin_temperature(
            self._h, s, background_temperature, int(bool(collisions)), _p(P),
            _p(T_s)))
        return P, T_s

    def lyman_alpha_emissivity(self):
        """W m^-3 of Lyman alpha from recombinations per cell, from the cells
        as they are (cmi_gpu_lyman_alpha_emissivity)"""
        out = np.zeros(self.n)
        self._check(self._lib.cmi_gpu_lyman_alpha_emissivity(self._h, _p(out)))
        return out

    def render_lyman_alpha_cube(self, theta, phi, nx, ny, anchor, sides,
                                npackets, seed, nchan, vmin, vmax,
                                sigma_turb=0., core_skip=0., dust=None,
                                source=None, max_scatter=LYA_MAX_SCATTER,
                                field=False):
        """The Lyman-alpha image (nx, ny) and cube (nchan, nx, ny) of one
        Monte Carlo run of `npackets` packets that scatter off the cells' H I
        (and off dust: `dust` = (sigma per hydrogen nucleus, albedo, g, p_l),
        None for none), both scaled by L_total / (npackets A_pixel): W m^-2
        sr^-1, per channel for the cube, the unit of
        render_scattered_line_cube. `source` is a luminosity density (ncell,)
        in W m^-3; None takes lyman_alpha_emissivity(). `core_skip` is
        x_crit. With sequences for theta and phi the views share one run:
        (nviews, nx, ny) and (nviews, nchan, nx, ny). With `field` the run
        also tallies the radiation field, and the dict of
        lya_radiation_field is returned as a third value. Replaces the
        engine's CCD image, dust and dust source, and leaves the mode off."""
        if dust is None:
            self.set_dust_scattering_per_hydrogen(0.5, 0., 0., 0.)
        else:
            sigma, albedo, g, p_l = dust
            self.set_dust_scattering_per_hydrogen(g, p_l, albedo, sigma)
        several, scaled = self._scattered_parallel_cameras(
            theta, phi, nx, ny, anchor, sides, npackets)
        self.set_cell_source_field(self.lyman_alpha_emissivity()
                                   if source is None else source)
        try:
            self.set_lyman_alpha(nchan, vmin, vmax, sigma_turb, core_skip,
                                 max_scatter)
            if field:
                self.set_lya_field(True)
            self.lya_shoot(seed, 0, int(npackets))
            total = self.get_cell_source(tables=False)
            images, cubes = self.download_lya()
            images = scaled(images, total)
            cubes = scaled(cubes, total)
            if field:
                field = self.lya_radiation_field(npackets, total)
        finally:
            self.set_lyman_alpha(0, 0., 1.)
        if not several:
            images, cubes = images[0], cubes[0]
        if field:
            return images, cubes, field
        return images, cubes

    def get_timing(self, reset=True):
        s = C.c_double()
        u = C.c_double()
        k = C.c_double()
        ns = C.c_uint64()
        nu = C.c_uint64()
        nk = C.c_uint64()
        self._check(self._lib.cmi_gpu_get_kernel_timing(
            self._h, C.byref(k), C.byref(nk)))
        self._check(self._lib.cmi_gpu_get_timing(
            self._h, int(reset), C.byref(s), C.byref(ns), C.byref(u),
            C.byref(nu)))
        return {"shoot_ms": s.value, "shoot_launches": ns.value,
                "update_ms": u.value, "update_launches": nu.value,
                "kernel_ms": k.value, "kernel_launches": nk.value}
