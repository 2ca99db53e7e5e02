"""The CPU restatement of the absorption spectra
(tests/support/absorption_reference.c) through ctypes - no GPU needed - and
what the absorption tests share: the numpy form of the contract's update, the
error bounds, the test box, its sightlines and its random lines."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import absorbing_cube_lib as A
import line_image_lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "support", "absorption_reference.c")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None
_p, _f64 = L._p, L._f64

EPS = A.EPS

# 11 x 9 x 7 cells with three different cell sides (0.25, 0.5, 0.375: exact in
# binary, so that walls, corners and diagonals are exact too)
BOX = L.Box((-1., 0.5, 2.), (2.75, 4.5, 2.625), (11, 9, 7))
NCHANS = (1, 63, 64, 65, 200, 300)
DV = 2.


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp) once per
    source version and load it."""
    global _lib
    if _lib is not None:
        return _lib
    digest = hashlib.sha256(open(SOURCE, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_absorption_reference_%d_%s.so" % (os.getuid(),
                                                              digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    lb = C.CDLL(out)
    axis = [C.c_int32, C.c_double, C.c_double]
    lb.abref_spectra.argtypes = [_dp, _dp, _ip, C.c_int32, _dp, _dp, _dp, _dp,
                                 _dp, C.c_int64, _dp, _dp, _dp, _dp] + axis + \
        [_dp, _dp]
    lb.abref_spectra.restype = C.c_int64
    lb.abref_probe.argtypes = [_dp, _dp, _ip, _dp, _dp, C.c_double,
                               C.c_double, _dp, _dp, _dp, C.c_double, _dp] + \
        axis + [C.c_int32, _ip, C.c_int32, _dp]
    lb.abref_probe.restype = None
    _lib = lb
    return lb


def _or_none(a):
    return None if a is None else _p(a)


longest_ray = 0


def spectra(box, n, b, S, g, origins, directions, lengths, nchan, vmin, vmax,
            velocity=None, observer_velocity=None):
    """tau (nrays, K, nchan) and N (nrays, K); longest_ray is set to the
    largest number of crossings of a ray"""
    global longest_ray
    S = _f64(S).reshape(-1)
    g = _f64(g).reshape(len(S))
    n = _f64(n).reshape(len(S), box.n)
    b = _f64(b).reshape(len(S), box.n)
    v = None if velocity is None else _f64(velocity).reshape(3, box.n)
    vo = None if observer_velocity is None else \
        _f64(observer_velocity).reshape(3)
    d = _f64(directions).reshape(-1, 3)
    o = _f64(np.broadcast_to(_f64(origins).reshape(-1, 3), d.shape))
    ln = _f64(np.broadcast_to(_f64(lengths).reshape(-1), (len(d),)))
    tau = np.zeros((len(d), len(S), nchan))
    N = np.zeros((len(d), len(S)))
    longest_ray = lib().abref_spectra(
        *box._args(), len(S), _p(n), _p(b), _p(S), _p(g), _or_none(v), len(d),
        _p(o), _p(d), _p(ln), _or_none(vo), nchan, vmin, vmax, _p(tau), _p(N))
    return tau, N


def probe(box, n, b, S, g, origin, direction, max_cells, nchan, vmin, vmax,
          channels=(), length=np.inf, velocity=None, observer_velocity=None):
    """the row of GpuEngine.absorption_probe"""
    n = _f64(n).reshape(box.n)
    b = _f64(b).reshape(box.n)
    v = None if velocity is None else _f64(velocity).reshape(3, box.n)
    vo = None if observer_velocity is None else \
        _f64(observer_velocity).reshape(3)
    ch = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
    out = np.zeros(3 + (2 + len(ch)) * max_cells + len(ch))
    lib().abref_probe(*box._args(), _p(n), _p(b), S, g, _or_none(v),
                      _p(_f64(origin).reshape(3)),
                      _p(_f64(direction).reshape(3)), length, _or_none(vo),
                      nchan, vmin, vmax, len(ch), ch.ctypes.data_as(_ip),
                      max_cells, _p(out))
    return out


def split_probe(row, max_cells, nprobe):
    """t0, t1, steps, cells, ds, tau[nprobe][max_cells], tau_end[nprobe]"""
    m = max_cells
    return (row[0], row[1], int(row[2]), row[3:3 + m].astype(np.int64),
            row[3 + m:3 + 2 * m],
            row[3 + 2 * m:3 + (2 + nprobe) * m].reshape(nprobe, m),
            row[3 + (2 + nprobe) * m:])


# the contract in numpy --------------------------------------------------------
def wing_Q(a, x2):
    """the wing term of Tasitsiomi (2006), the contract's form"""
    x2 = np.asarray(x2, dtype=np.float64)
    z = (x2 - 0.855) / (x2 + 3.42)
    with np.errstate(divide="ignore", invalid="ignore"):
        Q = (1. + 21. / x2) * a / (np.pi * (x2 + 1.)) * \
            (z * (0.1117 + z * (4.421 + z * (-9.207 + 5.674 * z))))
    return np.where(z > 0., Q, 0.)


def crossing_tau(n, ds, S, g, b, u, nchan, vmin, vmax):
    """what one crossing adds to tau[nchan], with scipy-free erf (math.erf)"""
    import math
    dv = (vmax - vmin) / nchan
    e = vmin + np.arange(nchan + 1) * dv
    E = np.array([1. if z >= 6. else (math.erf(z) if z > -6. else -1.)
                  for z in (e - u) / b])
    f = 0.5 * (E[1:] - E[:-1])
    A = (n * ds) * S
    if g == 0.:
        return A * (f / dv)
    x = (0.5 * (e[:-1] + e[1:]) - u) / b
    return A * (f / dv + wing_Q(g / b, x * x) / b)


# The largest value of Q(1, x^2) (Q is linear in a): from the formula on a fine
# grid of x; it is reached near x = 1.9.
_X = np.linspace(0.9, 30., 200001)
Q_MAX = float(np.max(wing_Q(1., _X * _X)))


# the bounds -------------------------------------------------------------------
# Device and restatement run the same IEEE operations in the same order on the
# same cells and path lengths (the probes show that cells and ds agree
# exactly): nds, A, u, the arguments z = (e - u) / b, x, a = g / b and the
# wing term, which is made of +, -, * and / only, are the same bits on both
# sides. They differ where erf does. As in absorbing_cube_lib the device's erf
# is within U_DEV = 4 ulps, glibc's within U_CPU = 1, an ulp of a value of at
# most 1 is at most 2 EPS and f = 0.5 (E_hi - E_lo) has two of them:
#   |f_gpu - f_cpu| <= DF = 2 (U_DEV + U_CPU) EPS = 10 EPS
# absolutely, however small f is; where the clamp or b == 0 makes E +-1 they
# agree exactly. With AD = the largest n ds S / dv of the call (ds at most the
# diagonal of a cell) a crossing's term A (f / dv + wing) differs by at most
# AD DF through f. From there on the two sides round different numbers: the
# quotient f / dv, the sum with the wing and the product with A are three
# roundings a side, 6 EPS of the term, and the sum into tau one a side, 2 EPS
# of the running tau. All terms are >= 0, so the terms of a channel sum to at
# most its tau and the running tau is at most the final one:
#   |tau_gpu - tau_cpu| <= (crossings (AD DF + 2 tau) + 6 tau) EPS
# an absolute part of order crossings AD 10 EPS and a relative part, which is
# what the wings of a damped line see. N has no erf in it: exact.
DF_EPS = A.DF_EPS


def line_depth(box, n, S, dv):
    """AD per line: max(n) S / dv times the diagonal of a cell"""
    diagonal = float(np.sqrt((box.cellside ** 2).sum()))
    return np.max(_f64(n).reshape(len(_f64(S).reshape(-1)), -1), axis=1) * \
        _f64(S).reshape(-1) / dv * diagonal


def parity_bound(crossings, AD, tau):
    """the bound above for tau[..., K, nchan] with AD[K]"""
    AD = np.asarray(AD, dtype=np.float64)[:, None]
    return (crossings * (AD * DF_EPS + 2. * tau) + 6. * tau) * EPS


def wing_depth(n, b, S, g):
    """the largest n S wing of a cell per line, m^-1: wing = Q(g / b, x^2) / b
    <= (g / b) Q_MAX / b"""
    n, b = _f64(n), _f64(b)
    out = np.zeros(len(n))
    for l in range(len(n)):
        ok = (n[l] > 0.) & (b[l] > 0.)
        if g[l] > 0. and ok.any():
            out[l] = np.max(n[l][ok] * S[l] * g[l] * Q_MAX / b[l][ok] ** 2)
    return out


# random lines of the parity tests ---------------------------------------------
# S of the three lines; g: none, a of about 5e-4 and a strongly damped one of
# about 0.05 at the typical b = DV
LINE_S = np.array([3e-6, 1e-6, 2e-5])
LINE_G = np.array([0., 5e-4 * DV, 0.05 * DV])


def random_lines(box, seed, dv=DV, tau_lo=1e-12, tau_hi=50.):
    """n[3][ncell], b[3][ncell], velocity[3][ncell]: n ds S / dv of a cell
    log-uniform in [tau_lo, tau_hi] (ds the mean cell side) with a tenth of
    the cells exactly 0; b from a tenth of a channel to four channels, and for
    the g == 0 line a tenth of the cells with b == 0, half of them at rest so
    that they sit exactly on an edge of an axis that has one at 0; random
    velocities of a few channels"""
    rng = np.random.default_rng(seed)
    ds = float(box.cellside.mean())
    K, ncell = len(LINE_S), box.n
    depth = np.exp(rng.uniform(np.log(tau_lo), np.log(tau_hi), (K, ncell)))
    depth[rng.random((K, ncell)) < 0.1] = 0.
    n = depth / ds * dv / LINE_S[:, None]
    b = dv * 10. ** rng.uniform(-1., np.log10(4.), (K, ncell))
    cold = rng.random(ncell) < 0.1
    b[0][cold] = 0.
    velocity = rng.normal(size=(3, ncell)) * 3. * dv
    on_edge = cold & (rng.random(ncell) < 0.5)
    velocity[:, on_edge] = 0.
    return n, b, velocity


def default_rows():
    """R, the slab rows per wave of a long axis (absorption_kernels.h)"""
    import re
    text = open(os.path.join(L.ROOT, "cmacionize_amd", "csrc",
                             "absorption_kernels.h")).read()
    return int(re.search(r"#define CMI_ABSORPTION_R (\d+)", text).group(1))


def axis_of(nchan, dv=DV):
    """nchan channels of width dv with an edge at exactly 0"""
    vmin = -dv * (nchan // 2)
    return nchan, vmin, vmin + dv * nchan


def sightlines(box):
    """the 12 sightlines of the tests: origins, unit directions, lengths"""
    a, s, c = box.anchor, box.sides, box.cellside
    hi = a + s
    r3 = 1. / np.sqrt(3.)
    mid = a + c * np.array([5.5, 4.5, 3.5])
    rays = [
        # along +x through cell centres, from outside, to the edge
        ((a[0] - 1., mid[1], mid[2]), (1., 0., 0.), np.inf),
        # along -z, ending inside a cell
        ((mid[0], mid[1], hi[2] + 0.5), (0., 0., -1.), 0.5 + 2.3 * c[2]),
        # along +y, ending exactly on a cell wall
        ((mid[0], a[1] - 0.5, mid[2]), (0., 1., 0.), 0.5 + 3. * c[1]),
        # the exact diagonal of a cube of cells' corners is no diagonal of
        # these cells (three sides); a diagonal in the x-z plane through the
        # corners of 3 x 2 blocks of cells (0.75 : 0.75) ties at every third
        ((a[0] - 0.75, mid[1], a[2] - 0.75), (np.sqrt(0.5), 0., np.sqrt(0.5)),
         np.inf),
        # the space diagonal direction from the box's lower corner
        (a - 0.5, (r3, r3, r3), np.inf),
        # an origin inside the box, a generic direction, a length inside
        (a + s * np.array([0.37, 0.52, 0.61]), (0.48, -0.6, 0.64), 1.1),
        # the same to the edge
        (a + s * np.array([0.37, 0.52, 0.61]), (0.48, -0.6, 0.64), np.inf),
        # an origin on the upper x wall pointing outwards
        ((hi[0], mid[1], mid[2]), (1., 0., 0.), np.inf),
        # a ray that misses the box
        ((a[0] - 1., a[1] - 1., mid[2]), (0., -1., 0.), np.inf),
        # a length that ends before the box
        ((a[0] - 1., mid[1], mid[2]), (1., 0., 0.), 0.75),
        # a length beyond the box
        ((a[0] - 1., mid[1] + 0.1, mid[2]), (0.8, 0.6, 0.), 50.),
        # an origin on a cell wall inside, generic direction
        ((a[0] + 4. * c[0], mid[1], mid[2]), (-0.36, 0.48, 0.8), 2.),
    ]
    o = _f64([r[0] for r in rays])
    d = _f64([r[1] for r in rays])
    ln = _f64([r[2] for r in rays])
    return o, d, ln
