"""The CPU restatement of the continuum images
(tests/support/continuum_reference.c) through ctypes - no GPU needed - and
what the continuum tests share: the numpy form of the free-free coefficients,
the error bound of a march, the test box and its rays."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import line_cube_lib as LC
import line_image_lib as L
import sky_image_lib as S

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "support", "continuum_reference.c")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None
_p, _f64 = L._p, L._f64

# the cube tests' shapes
BOX, NX, NY, VIEWS = LC.BOX, LC.NX, LC.NY, LC.VIEWS
image_rectangle = LC.image_rectangle

# the constants of csrc/device_common.h, the same literals
PLANCK = 6.626070040e-34
BOLTZMANN = 1.38064852e-23
LIGHTSPEED = 299792458.
FREE_FREE = 5.444364709e-52

EPS = 2. ** -53  # the relative error of one correctly rounded operation


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp) once per
    source version and load it."""
    global _lib
    if _lib is not None:
        return _lib
    digest = hashlib.sha256(open(SOURCE, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_continuum_reference_%d_%s.so" % (os.getuid(),
                                                             digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    lb = C.CDLL(out)
    lb.kref_images.argtypes = [_dp, _dp, _ip, C.c_double, C.c_double,
                               C.c_int32, C.c_int32, _dp, _dp, C.c_int32,
                               C.c_int32, _dp, _dp, _dp, _dp]
    lb.kref_images.restype = C.c_int64
    lb.kref_sky.argtypes = [_dp, _dp, _ip, _dp, C.c_int64, _dp, C.c_int32,
                            _dp, _dp, _dp, _dp]
    lb.kref_sky.restype = C.c_int64
    lb.kref_probe.argtypes = [_dp, _dp, _ip, C.c_int32, _dp, C.c_int64, _dp,
                              C.c_int32, _dp, _dp, _dp, C.c_int32, _dp]
    lb.kref_probe.restype = None
    _lib = lb
    return lb


def _channels(box, kappa, source, background):
    k = _f64(kappa).reshape(-1, box.n)
    s = _f64(source).reshape(len(k), box.n)
    bg = None if background is None else \
        _f64(np.broadcast_to(_f64(background), (len(k),)))
    return k, s, bg


longest_ray = 0


def images(box, kappa, source, theta, phi, nx, ny, anchor, sides,
           supersample=1, background=None):
    """(nf, nx, ny) of the parallel camera; longest_ray is set to the largest
    number of crossings of a sample ray"""
    global longest_ray
    k, s, bg = _channels(box, kappa, source, background)
    a = _f64(anchor).reshape(2)
    sd = _f64(sides).reshape(2)
    out = np.zeros((len(k), nx, ny))
    longest_ray = lib().kref_images(
        *box._args(), theta, phi, nx, ny, _p(a), _p(sd), supersample, len(k),
        _p(k), _p(s), _p(bg) if bg is not None else None, _p(out))
    return out


def sky(box, kappa, source, origin, directions, background=None):
    """(nf, nrays) of the rays from a point"""
    global longest_ray
    k, s, bg = _channels(box, kappa, source, background)
    o = _f64(origin).reshape(3)
    d = _f64(directions).reshape(-1, 3)
    out = np.zeros((len(k), len(d)))
    longest_ray = lib().kref_sky(
        *box._args(), _p(o), len(d), _p(d), len(k), _p(k), _p(s),
        _p(bg) if bg is not None else None, _p(out))
    return out


def probe(box, kappa, source, rays, max_cells, theta=None, phi=None,
          origin=None, background=None):
    """rows {t0, t1, steps, cells[max_cells], ds[max_cells],
    I[nf][max_cells], I_end[nf]}"""
    k, s, bg = _channels(box, kappa, source, background)
    point = origin is not None
    view = _f64(origin).reshape(3) if point else _f64([theta, phi])
    r = _f64(rays).reshape(-1, 3 if point else 2)
    nf = len(k)
    out = np.zeros((len(r), 3 + (2 + nf) * max_cells + nf))
    lib().kref_probe(*box._args(), int(point), _p(view), len(r), _p(r), nf,
                     _p(k), _p(s), _p(bg) if bg is not None else None,
                     max_cells, _p(out))
    return out


def split_probe(rows, nf, max_cells):
    """(t, steps, cells, ds, I[n][nf][max_cells], I_end[n][nf]) of probe
    rows"""
    m = max_cells
    return (rows[:, :2], rows[:, 2].astype(np.int64), rows[:, 3:3 + m],
            rows[:, 3 + m:3 + 2 * m],
            rows[:, 3 + 2 * m:3 + (2 + nf) * m].reshape(len(rows), nf, m),
            rows[:, 3 + (2 + nf) * m:])


# the bound of the parity tests -----------------------------------------------
# Device and restatement run the same IEEE operations on the same cells and
# path lengths (the probes show that those agree exactly), so they differ
# only where expm1 does. The ROCm device library documents its fp64 expm1
# within 1 ulp and glibc documents its own within 1 ulp, which puts the two
# values of em at most EXPM1_ULPS = 2 ulps apart: em_d = em_r (1 + h) with
# |h| <= 2 * 2^-52 = 4 EPS, EPS = 2^-53 the relative error of one rounding.
# M = max(|S|, |bg|) bounds every |I| (a convex combination of S and bg, up
# to terms of second order in EPS, which are dropped throughout).
#
# Parallel camera, I' = I + em (I - S) = (1 + em) I - em S, -1 <= em <= 0.
# Two marches a distance d apart before the step are afterwards at most
#   (1 + em) d          what is there already is not amplified
#   + |em| h |I - S|    <= 4 EPS * 2 M = 8 M EPS from expm1
#   + roundings         per march: the difference (2 M EPS), the product
#                       (its own 2 M EPS and the difference's, 2 M EPS) and
#                       the sum (M EPS), 5 M EPS; two marches, 10 M EPS
# apart: 18 M EPS per crossing.
#
# Rays from a point, I' = I + T (S (-em)), T' = T + T em. Every error T
# picks up in a step is proportional to the T it has: 4 EPS T from expm1 and
# 2 EPS T of roundings per march, 8 EPS T_j at step j, carried on times the
# product P of the later (1 + em). What that does to I is the sum over later
# steps i of dT_i |em_i| M, and sum_i |em_i| P(j..i) telescopes to at most 1:
# at most 8 M EPS per crossing. I's own terms per crossing are T |S em| h <=
# 4 M EPS and three roundings per march (two products and the sum), 6 M EPS
# for two. The last step I + T bg adds dT_n M <= 8 n M EPS and two roundings
# per march, 4 M EPS. In all (8 + 4 + 6 + 8) = 26 M EPS per crossing, and
# 4 M EPS once.
#
# The average of s^2 samples of which each is within d: d, and the roundings
# of s^2 additions and one division per side, 2 (s^2 + 1) M EPS.
EXPM1_ULPS = 2
STEP_EPS_PARALLEL = 2. * EXPM1_ULPS * 2. + 10.
STEP_EPS_POINT = 8. + 2. * EXPM1_ULPS + 6. + 8.


def march_bound(crossings, source, background, point=False, supersample=1):
    """the largest absolute difference a march of `crossings` cells may show
    between device and restatement (see above)"""
    m = max(float(np.max(np.abs(source))),
            float(np.max(np.abs(background))) if background is not None
            else 0.)
    per_step = STEP_EPS_POINT if point else STEP_EPS_PARALLEL
    once = 4. if point else 2. * (supersample * supersample + 1)
    return (per_step * int(crossings) + once) * m * EPS


# the free-free coefficients in numpy -----------------------------------------
def free_free(n, T, x_H0, x_He0, A_He, nu):
    """kappa[nf][ncell], S[nf][ncell]: the contract's formulas, operation
    for operation"""
    n, T, x_H0, x_He0 = (np.asarray(a, dtype=np.float64).reshape(-1)
                         for a in (n, T, x_H0, x_He0))
    nu = np.asarray(nu, dtype=np.float64).reshape(-1)
    kappa = np.zeros((len(nu), len(n)))
    source = np.zeros((len(nu), len(n)))
    n_e = n * ((1. - x_H0) + A_He * (1. - x_He0))
    ok = (n_e != 0.) & (T > 0.)
    Tk, ne = T[ok], n_e[ok]
    for f, v in enumerate(nu):
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            x = (PLANCK * v) / (BOLTZMANN * Tk)
            S = (2. * PLANCK * v * v * v / (LIGHTSPEED * LIGHTSPEED)) / \
                np.expm1(x)
            g = np.log(np.exp(5.960 - (np.sqrt(3.) / np.pi) *
                              np.log((v / 1.e9) * np.power(Tk / 1.e4, -1.5)))
                       + np.e)
            j = FREE_FREE * g * ne * ne / np.sqrt(Tk) * np.exp(-x)
            k = np.where(S == 0., 0., j / np.where(S == 0., 1., S))
        kappa[f, ok] = k
        source[f, ok] = S
    return kappa, source


def gaunt(nu, T):
    return np.log(np.exp(5.960 - (np.sqrt(3.) / np.pi) *
                         np.log((nu / 1.e9) * np.power(T / 1.e4, -1.5)))
                  + np.e)


# rays of the sky tests -------------------------------------------------------
def sky_origins(box):
    """an origin inside a cell, one on a cell wall and one outside the box"""
    inside = box.anchor + box.sides * np.array([0.37, 0.52, 0.61])
    wall = inside.copy()
    wall[0] = box.anchor[0] + box.cellside[0] * 5
    outside = box.anchor + box.sides * np.array([1.4, 0.3, -0.2])
    return [inside, wall, outside]


def sky_directions(seed=11, n=474, box=None, origin=None):
    """the 26 axis-parallel and diagonal unit vectors and n random ones; with
    a box and an origin half of the random ones aim at points of the box, so
    that an observer outside it has rays that hit it"""
    rng = np.random.default_rng(seed)
    d = S.random_directions(rng, n)
    if origin is not None:
        towards = box.anchor + box.sides * rng.uniform(0., 1., (n // 2, 3)) - \
            _f64(origin)
        d[:n // 2] = towards / np.sqrt((towards * towards).sum(axis=1))[:, None]
    return np.concatenate([S.special_directions(), d])


def random_channels(box, nf, seed, tau_lo=1e-12, tau_hi=50.,
                    zero_fraction=0.1):
    """kappa[nf][ncell] with the optical depth of a cell log-uniform in
    [tau_lo, tau_hi] and a tenth of the cells exactly 0, S[nf][ncell] and
    bg[nf] uniform in [0.5, 2] times a scale of their own per channel"""
    rng = np.random.default_rng(seed)
    ds = float(box.cellside.mean())
    tau = np.exp(rng.uniform(np.log(tau_lo), np.log(tau_hi),
                             size=(nf, box.n)))
    tau[rng.random((nf, box.n)) < zero_fraction] = 0.
    scale = 10. ** rng.uniform(-20., -16., size=(nf, 1))
    source = scale * rng.uniform(0.5, 2., size=(nf, box.n))
    bg = scale[:, 0] * rng.uniform(0.5, 2., size=nf)
    return tau / ds, source, bg


def driver_frequencies(n, nu_min, nu_max):
    """the frequencies `cmi-gpu --emission` makes of its continuum keys"""
    if n == 1:
        return np.array([float(nu_min)])
    return np.array([nu_min * np.power(nu_max / nu_min, f / (n - 1.))
                     for f in range(n)])


def channel_block():
    """FB, the channels per march launch (continuum_kernels.h)"""
    import re
    text = open(os.path.join(L.ROOT, "cmacionize_amd", "csrc",
                             "continuum_kernels.h")).read()
    return int(re.search(r"#define CMI_CONTINUUM_FB (\d+)", text).group(1))
