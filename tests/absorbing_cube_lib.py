"""The CPU restatement of the absorbing line cubes
(tests/support/absorbing_cube_reference.c) through ctypes - no GPU needed -
and what the absorbing cube tests share: the numpy form of the 21-cm
coefficients, the error bound of a march, the test box and random fields."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import continuum_lib as K
import line_cube_lib as LC
import line_image_lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "support", "absorbing_cube_reference.c")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None
_p, _f64 = L._p, L._f64

# the cube tests' shapes
BOX, NX, NY, VIEWS = LC.BOX, LC.NX, LC.NY, LC.VIEWS
image_rectangle = LC.image_rectangle
sky_origins, sky_directions = K.sky_origins, K.sky_directions

# the constants of csrc/device_common.h and csrc/absorbing_cube_kernels.h,
# the same literals
PLANCK, BOLTZMANN, LIGHTSPEED = K.PLANCK, K.BOLTZMANN, K.LIGHTSPEED
ATOMIC_MASS_UNIT = 1.660539040e-27
HYDROGEN_WEIGHT = 1.00794
HI_FREQUENCY = 1420405751.768
HI_EINSTEIN_A = 2.8843e-15
HI_COLUMN_CONSTANT = 5.516606267115072e-20

EPS = 2. ** -53  # the relative error of one correctly rounded operation


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp) once per
    source version and load it."""
    global _lib
    if _lib is not None:
        return _lib
    digest = hashlib.sha256(open(SOURCE, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_absorbing_cube_reference_%d_%s.so" % (os.getuid(),
                                                                  digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    lb = C.CDLL(out)
    fields = [_dp] * 7
    axis = [C.c_int32, C.c_double, C.c_double]
    lb.aref_cube.argtypes = [_dp, _dp, _ip, C.c_double, C.c_double, C.c_int32,
                             C.c_int32, _dp, _dp, C.c_int32] + fields + \
        axis + [_dp]
    lb.aref_cube.restype = C.c_int64
    lb.aref_sky_cube.argtypes = [_dp, _dp, _ip, _dp, _dp, C.c_int64, _dp] + \
        fields + axis + [_dp]
    lb.aref_sky_cube.restype = C.c_int64
    lb.aref_probe.argtypes = [_dp, _dp, _ip, C.c_int32, _dp, _dp, C.c_int64,
                              _dp] + fields + axis + [C.c_int32, _dp]
    lb.aref_probe.restype = None
    _lib = lb
    return lb


def _or_none(a):
    return None if a is None else _p(a)


def _fields(box, a, sl, b, velocity, kc, sc, background, nchan):
    """the seven arrays as the restatement takes them (kept alive by the
    caller's list)"""
    arrays = [_f64(a).reshape(box.n), _f64(sl).reshape(box.n),
              _f64(b).reshape(box.n),
              None if velocity is None else _f64(velocity).reshape(3, box.n),
              None if kc is None else _f64(kc).reshape(box.n),
              None if sc is None else _f64(sc).reshape(box.n),
              None if background is None else
              _f64(np.broadcast_to(_f64(background), (nchan,)))]
    return arrays


longest_ray = 0


def cube(box, a, sl, b, theta, phi, nx, ny, anchor, sides, nchan, vmin, vmax,
         supersample=1, velocity=None, kc=None, sc=None, background=None):
    """(nchan, nx, ny) of the parallel camera; longest_ray is set to the
    largest number of crossings of a sample ray"""
    global longest_ray
    f = _fields(box, a, sl, b, velocity, kc, sc, background, nchan)
    an = _f64(anchor).reshape(2)
    sd = _f64(sides).reshape(2)
    out = np.zeros((nchan, nx, ny))
    longest_ray = lib().aref_cube(
        *box._args(), theta, phi, nx, ny, _p(an), _p(sd), supersample,
        *[_or_none(x) for x in f], nchan, vmin, vmax, _p(out))
    return out


def sky_cube(box, a, sl, b, origin, directions, nchan, vmin, vmax,
             velocity=None, kc=None, sc=None, background=None,
             observer_velocity=None):
    """(nchan, nrays) of the rays from a point"""
    global longest_ray
    f = _fields(box, a, sl, b, velocity, kc, sc, background, nchan)
    o = _f64(origin).reshape(3)
    d = _f64(directions).reshape(-1, 3)
    vo = None if observer_velocity is None else \
        _f64(observer_velocity).reshape(3)
    out = np.zeros((nchan, len(d)))
    longest_ray = lib().aref_sky_cube(
        *box._args(), _p(o), _or_none(vo), len(d), _p(d),
        *[_or_none(x) for x in f], nchan, vmin, vmax, _p(out))
    return out


def probe(box, a, sl, b, rays, max_cells, nchan, vmin, vmax, theta=None,
          phi=None, origin=None, velocity=None, kc=None, sc=None,
          background=None, observer_velocity=None):
    """rows {t0, t1, steps, cells[max_cells], ds[max_cells],
    I[nchan][max_cells], I_end[nchan]}"""
    f = _fields(box, a, sl, b, velocity, kc, sc, background, nchan)
    point = origin is not None
    view = _f64(origin).reshape(3) if point else _f64([theta, phi])
    vo = None if observer_velocity is None else \
        _f64(observer_velocity).reshape(3)
    r = _f64(rays).reshape(-1, 3 if point else 2)
    out = np.zeros((len(r), 3 + (2 + nchan) * max_cells + nchan))
    lib().aref_probe(*box._args(), int(point), _p(view), _or_none(vo), len(r),
                     _p(r), *[_or_none(x) for x in f], nchan, vmin, vmax,
                     max_cells, _p(out))
    return out


split_probe = K.split_probe


# the bound of the parity tests -----------------------------------------------
# Device and restatement run the same IEEE operations on the same cells, path
# lengths and arguments z = (e - u) / b (e, u and b come from the same
# operations on the same inputs on both sides; the probes show that cells and
# ds agree exactly), so they differ only where expm1 and erf do.
#
# expm1: as in continuum_lib, the two values are at most EXPM1_ULPS = 2 ulps
# apart, a relative 4 EPS (EPS = 2^-53, the relative error of one rounding).
#
# erf: the device's is within U_DEV = 4 ulps (measured for the spectral line
# cubes and doubled), glibc's within U_CPU = 1; an ulp of a
# value of at most 1 is at most 2 EPS, and f = 0.5 (E_hi - E_lo) has two of
# them, so the two f differ by at most
#   DF = 2 (U_DEV + U_CPU) EPS = 10 EPS
# absolutely, however small f is. Where the clamp or b == 0 makes E +-1 the
# two agree exactly. That is an absolute difference adv DF of al and of kappa
# (adv = a / dv), and with A = the largest adv ds of the call (ds at most the
# diagonal of a cell) a difference of at most A DF of a cell's optical depth.
#
# M = max(|sl|, |sc|, |bg|) bounds every |S| (S lies between sc and sl, w in
# [0, 1]) and every |I| (a convex combination of S and bg); terms of second
# order in EPS are dropped.
#
# What a crossing adds to the distance d of two marches of the parallel
# camera, I' = I + em (I - S) = (1 + em) I - em S, -1 <= em <= 0:
#   (1 + em) d           what is there already is not amplified
#   f through em         |d em / d tau| = e^-tau <= 1, |I - S| <= 2 M:
#                        2 M A DF = 20 A M EPS
#   f through S          S = sc + w (sl - sc), w = al / kappa. Exactly,
#                        w_1 - w_2 = kc (al_1 - al_2) / (kappa_1 kappa_2), and
#                        |em_1| <= kappa_1 ds, so |em_1| |S_1 - S_2| <= 2 M ds
#                        |al_1 - al_2| (kc / kappa_2) <= 2 M A DF = 20 A M EPS
#                        (this holds however small kappa is, which is why the
#                        bound does not blow up where line and continuum are
#                        both thin; a channel that one side skips because its
#                        kappa is exactly 0 moves the other side by at most
#                        |em| 2 M <= 2 M A DF as well)
#   expm1                4 EPS |em| |I - S| <= 8 M EPS
#   roundings per march  of al, kappa and kappa ds: 3 EPS of tau, and |d em|
#                        <= |em| |d tau / tau|, 3 EPS 2 M = 6 M EPS; of w (al,
#                        kappa twice, the quotient: 4 EPS), of sl - sc and of
#                        the product (1 EPS each) on |w (sl - sc)| <= 2 M and
#                        of the sum on |S| <= M: 13 M EPS; of the update as in
#                        continuum_lib 5 M EPS; 24 M EPS, for two marches 48
# in all (56 + 40 A) M EPS per crossing.
#
# Rays from a point, I' = I + T (S (-em)), T' = T + T em. Every error T picks
# up in a step is proportional to the T it has: expm1 and the roundings of tau
# of both marches (4 + 6) EPS, the product and the sum of both marches 4 EPS,
# f through tau A DF = 10 A EPS: (14 + 10 A) EPS T_j at step j, carried on
# times the product of the later (1 + em). As in continuum_lib that reaches I
# through the later steps (the sum telescopes to at most 1) and through the
# last step I + T bg, twice (14 + 10 A) M EPS per crossing. I's own terms per
# crossing: T |S em| (4 + 6) EPS <= 10 M EPS; the roundings of S of two
# marches 26 M EPS; f through S 20 A M EPS and through em M A DF = 10 A M EPS;
# three roundings per march 6 M EPS. In all (70 + 50 A) M EPS per crossing,
# and 4 M EPS once for the last step.
#
# The average of s^2 samples of which each is within d: d, and the roundings
# of s^2 additions and one division per side, 2 (s^2 + 1) M EPS.
EXPM1_ULPS = K.EXPM1_ULPS
U_DEV = 4.   # tests/test_gpu_line_cube.py
U_CPU = 1.
DF_EPS = 2. * (U_DEV + U_CPU)


def line_depth(box, a, dv):
    """A: the largest whole-line optical depth a crossing of one cell can
    have, max(a / dv) times the diagonal of a cell"""
    diagonal = float(np.sqrt((box.cellside ** 2).sum()))
    return float(np.max(_f64(a))) / dv * diagonal


def march_bound(crossings, A, sl, sc, background, point=False, supersample=1):
    """the largest absolute difference a march of `crossings` cells may show
    between device and restatement (see above)"""
    m = max(float(np.max(np.abs(sl))),
            float(np.max(np.abs(sc))) if sc is not None else 0.,
            float(np.max(np.abs(background))) if background is not None
            else 0.)
    h = 2. * EXPM1_ULPS
    if point:
        per_step = (2. * (h + 6. + 4. + DF_EPS * A) + (h + 6.) + 26. +
                    3. * DF_EPS * A + 6.)
        once = 4.
    else:
        per_step = 2. * h + 48. + 4. * DF_EPS * A
        once = 2. * (supersample * supersample + 1)
    return (per_step * int(crossings) + once) * m * EPS


# the 21-cm coefficients in numpy ---------------------------------------------
def planck(nu, T):
    """B_nu(T) in the contract's form; 0 for T <= 0"""
    T = np.asarray(T, dtype=np.float64)
    out = np.zeros(T.shape)
    ok = T > 0.
    with np.errstate(over="ignore"):
        out[ok] = (2. * PLANCK * nu * nu * nu / (LIGHTSPEED * LIGHTSPEED)) / \
            np.expm1((PLANCK * nu) / (BOLTZMANN * T[ok]))
    return out


def hi_coefficients(n, T, x_H0, x_He0, A_He, sigma_turb=0.,
                    spin_temperature=None, free_free=True):
    """{a, sl, b, kc, sc}: the contract's formulas, operation for operation"""
    n, T, x_H0, x_He0 = (np.asarray(q, dtype=np.float64).reshape(-1)
                         for q in (n, T, x_H0, x_He0))
    Ts = T if spin_temperature is None else \
        np.broadcast_to(np.asarray(spin_temperature, dtype=np.float64),
                        T.shape)
    n_HI = n * x_H0
    ok = (n_HI > 0.) & (T > 0.) & (Ts > 0.)
    a = np.zeros(T.shape)
    a[ok] = HI_COLUMN_CONSTANT * n_HI[ok] / Ts[ok]
    thermal = np.where(T > 0., BOLTZMANN * T /
                       (HYDROGEN_WEIGHT * ATOMIC_MASS_UNIT), 0.)
    b = np.sqrt(2. * (thermal + sigma_turb * sigma_turb))
    if free_free:
        kc, sc = K.free_free(n, T, x_H0, x_He0, A_He, [HI_FREQUENCY])
        kc, sc = kc[0], sc[0]
    else:
        kc, sc = np.zeros(T.shape), np.zeros(T.shape)
    return {"a": a, "sl": planck(HI_FREQUENCY, Ts), "b": b, "kc": kc,
            "sc": sc}


def host_planck(T):
    """B_nu10(T) with the expm1 of the C library, as the engine's host side
    forms the background of the H I calls"""
    import ctypes.util
    m = C.CDLL(ctypes.util.find_library("m"))
    m.expm1.argtypes = [C.c_double]
    m.expm1.restype = C.c_double
    if not T > 0.:
        return 0.
    nu = HI_FREQUENCY
    x = (PLANCK * nu) / (BOLTZMANN * T)
    return (2. * PLANCK * nu * nu * nu / (LIGHTSPEED * LIGHTSPEED)) / \
        m.expm1(x)


# random cells of the parity tests --------------------------------------------
def random_cells(box, seed, dv, tau_lo=1e-12, tau_hi=50.):
    """a, sl, b, velocity, kc, sc: the whole-line optical depth a ds / dv and
    the continuum's kc ds of a cell log-uniform in [tau_lo, tau_hi] (ds the
    mean cell side) with a tenth of the cells exactly 0 each; b from 0 (a
    tenth of the cells: delta lines, half of them exactly on a channel edge
    of an axis that starts at a multiple of dv) to several channels; sl and
    sc uniform in [0.5, 2] times a scale"""
    rng = np.random.default_rng(seed)
    ds = float(box.cellside.mean())
    n = box.n
    tau = np.exp(rng.uniform(np.log(tau_lo), np.log(tau_hi), n))
    tau[rng.random(n) < 0.1] = 0.
    a = tau / ds * dv
    tau_c = np.exp(rng.uniform(np.log(tau_lo), np.log(tau_hi), n))
    tau_c[rng.random(n) < 0.1] = 0.
    kc = tau_c / ds
    scale = 10. ** rng.uniform(-20., -16.)
    sl = scale * rng.uniform(0.5, 2., n)
    sc = scale * rng.uniform(0.5, 2., n)
    b = dv * 10. ** rng.uniform(-1., np.log10(4.), n)
    cold = rng.random(n) < 0.1
    b[cold] = 0.
    velocity = rng.normal(size=(3, n)) * 3. * dv
    # delta lines on an edge: at rest along every view only if v == 0, so
    # give those cells no velocity at all and let the axis start at an edge
    on_edge = cold & (rng.random(n) < 0.5)
    velocity[:, on_edge] = 0.
    return a, sl, b, velocity, kc, sc


def channel_block():
    """CB, the channels per march launch (absorbing_cube_kernels.h)"""
    import re
    text = open(os.path.join(L.ROOT, "cmacionize_amd", "csrc",
                             "absorbing_cube_kernels.h")).read()
    return int(re.search(r"#define CMI_ABSORBING_CB (\d+)", text).group(1))
