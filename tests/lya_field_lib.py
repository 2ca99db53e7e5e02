"""The CPU restatement of the Lyman-alpha radiation field
(tests/support/lya_field_reference.c, which builds on lyman_alpha_reference.c
and the restatements below it) through ctypes - no GPU needed - and what the
field's tests share: the coupling formula in numpy, the scenes and the bounds
of a comparison of rows."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import lyman_alpha_lib as Y
import scattered_line_lib as SL

SOURCE = os.path.join(Y.SUPPORT, "lya_field_reference.c")
COLUMNS = ("L", "S_H", "S_d", "G_x", "G_y", "G_z", "N_H", "N_d")
L_, S_H, S_D, G_X, N_H, N_D = 0, 1, 2, 3, 6, 7
PLANCK = 6.626070040e-34
LIGHTSPEED = 299792458.
HI_FREQUENCY = 1420405751.768
HI_EINSTEIN_A = 2.8843e-15
T_STAR = PLANCK * HI_FREQUENCY / Y.BOLTZMANN

_dp = C.POINTER(C.c_double)
_p = Y._p
_f64 = Y._f64
_lib = None


def lib():
    """Compile the restatement once per version of its sources and load it,
    as lyman_alpha_lib.lib does (whose library serves the model's setup: the
    module-wide state of this one is its own)."""
    global _lib
    if _lib is not None:
        return _lib
    subprocess.run(["make", "-s", "-C", SL.ORACLE], check=True)
    h = hashlib.sha256()
    for name in ("lya_field_reference.c", "lyman_alpha_reference.c",
                 "scattered_cube_reference.c", "scattered_sky_reference.c",
                 "scattered_line_reference.c", "dust_reference.c"):
        h.update(open(os.path.join(Y.SUPPORT, name), "rb").read())
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_lya_field_reference_%d_%s.so" %
                       (os.getuid(), h.hexdigest()[:16]))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                        "-o", tmp, SOURCE, "-L" + SL.ORACLE, "-lcmio",
                        "-Wl,-rpath," + SL.ORACLE, "-lm"], check=True)
        os.replace(tmp, out)
    L = C.CDLL(out)
    i32p = C.POINTER(C.c_int32)
    u64p = C.POINTER(C.c_uint64)
    L.dref_setup.argtypes = [_dp, _dp, i32p, _dp, _dp] + [C.c_double] * 6 + \
        [C.c_int32, C.c_int32, _dp, _dp] + [C.c_double] * 3
    L.slref_set_field.argtypes = [_dp, C.c_int64]
    L.slref_get_tables.argtypes = [_dp, _dp, _dp]
    L.slref_get_tables.restype = None
    L.lyaref_set.argtypes = [C.c_int32] + [C.c_double] * 4 + [C.c_uint64] + \
        [_dp] * 4 + [C.c_double, _dp]
    L.lyaref_set.restype = C.c_int64
    L.lyafref_shoot.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp, _dp,
                                u64p, _dp, _dp, _dp, _dp]
    L.lyafref_shoot.restype = None
    L.lyafref_scattering_rate.argtypes = [C.c_int64, _dp, _dp, C.c_double,
                                          C.c_double, _dp]
    L.lyafref_scattering_rate.restype = None
    L.lyafref_spin_temperature.argtypes = [C.c_int64, _dp, _dp, _dp, _dp,
                                           C.c_double, C.c_int32, _dp]
    L.lyafref_spin_temperature.restype = None
    _lib = L
    return L


class Run:
    """what FieldRestatement.shoot returns"""

    def __init__(self, image, cube, counters, rows, crossings, sums, margin):
        self.image, self.cube, self.counters = image, cube, counters
        self.rows, self.crossings, self.margin = rows, crossings, margin
        self.chord = float(sums[0])
        self.momentum = np.array(sums[1:4])
        self.walk_steps = int(sums[4])
        self.march_steps = int(sums[5])


class FieldRestatement:
    """One scene (lyman_alpha_lib.Scene) of the restatement with the field"""

    def __init__(self, scene):
        s, m = scene, scene.m
        self.s = s
        L = lib()
        ones = np.ones(m.n)
        rc = L.dref_setup(
            _p(m.anchor), _p(m.sides),
            m.ncell.ctypes.data_as(C.POINTER(C.c_int32)), _p(m.density),
            _p(ones), m.g, m.p_l, m.albedo, m.sigma, m.theta, m.phi, m.nx,
            m.ny, _p(m.img_anchor), _p(m.img_sides), 1., 1., 0.)
        assert rc == 0
        assert L.slref_set_field(_p(s.field), m.n) == 0
        self.invalid = L.lyaref_set(
            s.nchan, s.vmin, s.vmax, s.sigma_turb, s.x_crit, s.max_scatter,
            _p(m.density), _p(ones), _p(s.n_HI), _p(s.T),
            m.sigma if s.dust else 0.,
            None if s.velocity is None else _p(s.velocity))

    def total_luminosity(self):
        total = np.zeros(1)
        lib().slref_get_tables(_p(total), None, None)
        return float(total[0])

    def shoot(self, seed, first, n, crossings=False):
        s, m = self.s, self.s.m
        image = np.zeros((m.nx, m.ny))
        cube = np.zeros((s.nchan, m.nx, m.ny))
        rows = np.zeros((m.n, 8))
        cross = np.zeros(m.n) if crossings else None
        sums = np.zeros(6)
        margin = np.zeros(1)
        c = (C.c_uint64 * 7)()
        lib().lyafref_shoot(seed, first, n, _p(image), _p(cube), c, _p(rows),
                            None if cross is None else _p(cross), _p(sums),
                            _p(margin))
        counters = dict(zip(("nsteps", "nhydrogen", "ndust", "nrejections",
                             "natomics", "ncapped", "npackets"),
                            (int(v) for v in c)))
        return Run(image, cube, counters, rows, cross, sums,
                   float(margin[0]))

    def scattering_rate(self, rows, scale):
        P = np.zeros(self.s.m.n)
        lib().lyafref_scattering_rate(self.s.m.n, _p(_f64(rows)),
                                      _p(self.s.n_HI.reshape(-1)), scale,
                                      cell_volume(self.s.m), _p(P))
        return P


def cell_volume(model):
    return float(np.prod(model.sides / model.ncell))


def spin_temperature_c(T, n_HI, n_e, P, T_gamma, collisions):
    """the restatement's coupling formula on arrays"""
    T, n_HI, n_e, P = (_f64(np.broadcast_to(v, np.shape(T)).reshape(-1))
                       for v in (T, n_HI, n_e, P))
    out = np.zeros(len(T))
    lib().lyafref_spin_temperature(len(T), _p(T), _p(n_HI), _p(n_e), _p(P),
                                   T_gamma, int(collisions), _p(out))
    return out


def kappa_HH(T):
    """m^3 s^-1 (Kuhlen, Madau & Montgomery 2006)"""
    return 3.1e-17 * T ** 0.357 * np.exp(-32. / T)


def kappa_eH(T):
    """m^3 s^-1 (Liszt 2001), held outside 1 K .. 1e4 K"""
    lT = np.log10(np.minimum(np.maximum(T, 1.), 1.e4))
    return 1.e-6 * 10. ** (-9.607 + 0.5 * lT * np.exp(-lT ** 4.5 / 1800.))


def spin_temperature_numpy(T, n_HI, n_e, P, T_gamma, collisions):
    """the contract's formula in numpy, float64"""
    T, n_HI, n_e, P = (np.asarray(v, dtype=float) for v in (T, n_HI, n_e, P))
    with np.errstate(all="ignore"):
        C_10 = (n_HI * kappa_HH(T) + n_e * kappa_eH(T)) if collisions else 0.
        x = 4. * P * T_STAR / (27. * HI_EINSTEIN_A * T_gamma) + \
            (C_10 / HI_EINSTEIN_A) * (T_STAR / T_gamma)
        T_s = (1. + x) / (1. / T_gamma + x / T)
    return np.where(T > 0., T_s, T_gamma)


def coupling(T, n_HI, n_e, T_gamma, collisions, P=0.):
    """x_alpha + x_c"""
    C_10 = (n_HI * kappa_HH(T) + n_e * kappa_eH(T)) if collisions else 0.
    return 4. * P * T_STAR / (27. * HI_EINSTEIN_A * T_gamma) + \
        (C_10 / HI_EINSTEIN_A) * (T_STAR / T_gamma)


def row_bounds(scene, ref_rows, crossings, relative=1e-8):
    """The bound [ncell][8] on |device - restatement| of a run's rows.

    The walk of the two sides is the same sequence of crossings (the tests
    hold the counters equal); positions agree within 1e-9 of a cell side and x
    within 1e-9, the bounds of the traces (test_gpu_lyman_alpha.py). A
    crossing's term W ds kappa_H is then off by at most its own (d ds / ds + d
    kappa_H / kappa_H). |d ln H / d x| <= 2 max(|x|, 1 / |x|) <= 7 over the
    core and falls in the wing, so d kappa_H / kappa_H <= 1e-8: the relative
    part. d ds <= 2e-9 of a cell's diagonal whatever ds is - it matters where
    ds is small: a clipped corner, the backed-off last crossing - : the
    absolute part, 2e-9 diagonal times the cell's largest opacity (H <= 1) per
    crossing of the cell. L has the absolute part alone (and rounding); S_d's
    opacity is a constant of the cell; G's components cancel, so they are
    held relative to S_H + S_d of the cell; N_H and N_d are sums of weights
    forced * albedos, forced = 1 - exp(-tau_max) with tau_max within 16 eps of
    itself: 1e-12 relative."""
    m = scene.m
    diag = float(np.sqrt(((m.sides / m.ncell) ** 2).sum()))
    b = Y.doppler_width(scene.T.reshape(-1), scene.sigma_turb)
    k0 = scene.n_HI.reshape(-1) * Y.line_centre_cross_section(b)
    kd = m.density.reshape(-1) * (m.sigma if scene.dust else 0.)
    step = 2e-9 * diag * crossings
    r = np.abs(ref_rows)
    out = np.zeros_like(ref_rows)
    out[:, L_] = 1e-12 * r[:, L_] + step
    out[:, S_H] = relative * r[:, S_H] + step * k0
    out[:, S_D] = 1e-12 * r[:, S_D] + step * kd
    out[:, G_X:G_X + 3] = (relative * (r[:, S_H] + r[:, S_D]) +
                           step * (k0 + kd))[:, None]
    out[:, N_H] = 1e-12 * r[:, N_H]
    out[:, N_D] = 1e-12 * r[:, N_D]
    return out


def whole_run_bounds(ref_rows, relative=1e-8):
    """1e-8 of the element; G relative to S_H + S_d of the cell"""
    r = np.abs(ref_rows)
    out = relative * r
    out[:, G_X:G_X + 3] = (relative * (r[:, S_H] + r[:, S_D]))[:, None]
    return out


def identity_sigmas(a, b):
    """|mean(a - b)| in standard errors of the batch means; a and b are
    [nbatch] or [nbatch][k]"""
    d = np.asarray(a, dtype=float) - np.asarray(b, dtype=float)
    se = d.std(axis=0, ddof=1) / np.sqrt(len(d))
    return np.abs(d.mean(axis=0)) / se
