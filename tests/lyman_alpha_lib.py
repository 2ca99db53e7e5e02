"""The CPU restatement of the Lyman-alpha transfer
(tests/support/lyman_alpha_reference.c, which builds on
scattered_cube_reference.c and the restatements below it) through ctypes - no
GPU needed - and what the Lyman-alpha tests share: the exact Voigt function,
the scenes, and the same setup on a GpuEngine."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import scattered_cube_lib as Q
import scattered_line_lib as SL

SUPPORT = SL.SUPPORT
SOURCE = os.path.join(SUPPORT, "lyman_alpha_reference.c")
EINVAL, ESTATE = SL.EINVAL, SL.ESTATE
VOIGT, OPTICAL_DEPTH, SAMPLER, TRACE = 0, 1, 2, 3  # cmi_gpu_lya_probe kinds
HEADER, ROW = 6, 12  # a trace's columns
LAMBDA0 = 1215.67e-10
A21 = 6.265e8
BOLTZMANN = 1.38064852e-23
M_H = 1.00794 * 1.660539040e-27
MAX_SCATTER = 100000000

_dp = C.POINTER(C.c_double)
_lib = None
_p = SL._p
_f64 = SL._f64


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp, linked
    against oracle/libcmio.so) once per version of its sources and load it."""
    global _lib
    if _lib is not None:
        return _lib
    subprocess.run(["make", "-s", "-C", SL.ORACLE], check=True)
    h = hashlib.sha256()
    for name in ("lyman_alpha_reference.c", "scattered_cube_reference.c",
                 "scattered_sky_reference.c", "scattered_line_reference.c",
                 "dust_reference.c"):
        h.update(open(os.path.join(SUPPORT, name), "rb").read())
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_lyman_alpha_reference_%d_%s.so" %
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
    L.dref_pixel.restype = C.c_int64
    L.dref_pixel.argtypes = [_dp]
    L.slref_set_field.argtypes = [_dp, C.c_int64]
    L.slref_get_tables.argtypes = [_dp, _dp, _dp]
    L.slref_get_tables.restype = None
    L.lyaref_set.argtypes = [C.c_int32] + [C.c_double] * 4 + [C.c_uint64] + \
        [_dp] * 4 + [C.c_double, _dp]
    L.lyaref_set.restype = C.c_int64
    L.lyaref_records.argtypes = [_dp]
    L.lyaref_records.restype = None
    L.lyaref_voigt.argtypes = [C.c_int64, _dp, _dp]
    L.lyaref_voigt.restype = None
    L.lyaref_optical_depth.argtypes = [C.c_int64, _dp, _dp]
    L.lyaref_optical_depth.restype = None
    L.lyaref_sampler.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp, _dp,
                                 _dp]
    L.lyaref_sampler.restype = None
    L.lyaref_trace.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp,
                               C.c_int32, _dp]
    L.lyaref_trace.restype = None
    L.lyaref_shoot.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp, _dp,
                               _dp, u64p, _dp]
    L.lyaref_shoot.restype = None
    _lib = L
    return L


# ------------------------------------------------------------ physics --

def doppler_width(T, sigma_turb=0.):
    return np.sqrt(2. * (BOLTZMANN * np.asarray(T, dtype=float) / M_H +
                         sigma_turb ** 2))


def voigt_parameter(b):
    return A21 * LAMBDA0 / (4. * np.pi * b)


def line_centre_cross_section(b):
    """m^2 per atom"""
    return 3. * LAMBDA0 ** 3 * A21 / (8. * np.pi ** 1.5 * b)


def exact_voigt(a, x):
    """H(a, x) = Re w(x + i a): scipy's Faddeeva function if importable,
    otherwise H = (a / pi) int exp(-y^2) / ((x - y)^2 + a^2) dy by the
    substitution y = x + a tan(t), the trapezoidal rule on 400001 nodes"""
    x = np.asarray(x, dtype=float)
    try:
        from scipy.special import wofz
        return wofz(x + 1j * a).real
    except ImportError:
        t = np.linspace(-0.5 * np.pi, 0.5 * np.pi, 400001)[1:-1]
        out = np.empty(x.shape)
        for i, xi in enumerate(x.ravel()):
            y = xi + a * np.tan(t)
            out.ravel()[i] = np.sum(np.exp(-y * y)) * (t[1] - t[0]) / np.pi
        return out


def atom_density(u, x, a):
    """the normalised density of u_par at frequency x"""
    f = np.exp(-u * u) / ((x - u) ** 2 + a * a)
    return f * a / (np.pi * exact_voigt(a, np.array([x]))[0])


def static_sphere_median(a_tau0):
    """the median of |x| of Dijkstra et al. (2006)'s J(x) ~ x^2 / (1 +
    cosh(sqrt(2 pi^3 / 27) |x|^3 / (a tau_0)))"""
    x = np.linspace(0., 6. * a_tau0 ** (1. / 3.), 600001)
    j = x * x / (1. + np.cosh(np.sqrt(2. * np.pi ** 3 / 27.) * x ** 3 /
                              a_tau0))
    c = np.cumsum(j)
    return float(x[np.searchsorted(c, 0.5 * c[-1])])


# -------------------------------------------------------------- scenes --

class Scene:
    """Everything a run takes: scattered_line_lib's Model (grid, n_H = its
    density, dust, camera), the source field, n_HI and T per cell, the
    velocities (ncell, 3) or None, and the mode's arguments. `dust` False
    leaves the dust out (sigma_d = 0)."""

    def __init__(self, model, field, n_HI, T, nchan, vmin, vmax,
                 velocity=None, sigma_turb=0., x_crit=0.,
                 max_scatter=MAX_SCATTER, dust=True):
        self.m = model
        self.field = _f64(field).reshape(model.n)
        self.n_HI = _f64(n_HI).reshape(model.n)
        self.T = _f64(T).reshape(model.n)
        self.nchan, self.vmin, self.vmax = int(nchan), float(vmin), float(vmax)
        self.velocity = None if velocity is None else \
            _f64(_f64(velocity).reshape(-1, 3).T)  # [3][ncell]
        self.sigma_turb, self.x_crit = float(sigma_turb), float(x_crit)
        self.max_scatter = int(max_scatter)
        self.dust = bool(dust)

    def engine(self, views=None):
        """a GpuEngine with the scene set up and the mode on; `views`: a list
        of (theta, phi) for set_ccd_images in place of the model's camera"""
        m = self.m
        eng = SL.make_engine(m, self.field)
        if not self.dust:
            eng.set_dust_scattering_per_hydrogen(0.5, 0., 0., 0.)
        if views is not None:
            eng.set_ccd_images([v[0] for v in views], [v[1] for v in views],
                               m.nx, m.ny, m.img_anchor, m.img_sides)
        self.apply(eng)
        return eng

    def apply(self, eng):
        eng.set_cell_velocities(self.velocity)
        eng.set_lyman_alpha(self.nchan, self.vmin, self.vmax, self.sigma_turb,
                            self.x_crit, self.max_scatter, self.n_HI, self.T)


class Restatement:
    """One scene of the CPU restatement (module-wide state in the C code: the
    last one set up is in use)."""

    def __init__(self, scene):
        self.s = scene
        self.setup()

    def setup(self):
        s, m = self.s, self.s.m
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

    def pixel(self, x):
        return int(lib().dref_pixel(_p(_f64(x))))

    def records(self):
        out = np.zeros((self.s.m.n, 8))
        lib().lyaref_records(_p(out))
        return out

    def voigt(self, rows):
        rows = _f64(rows).reshape(-1, 4)
        out = np.zeros((len(rows), 2))
        lib().lyaref_voigt(len(rows), _p(rows), _p(out))
        return out

    def optical_depth(self, rows):
        rows = _f64(rows).reshape(-1, 7)
        out = np.zeros((len(rows), 2))
        lib().lyaref_optical_depth(len(rows), _p(rows), _p(out))
        return out

    def sampler(self, seed, first, rows):
        """{u_par, rejections} per row {x, a}, and the rows' margins"""
        rows = _f64(rows).reshape(-1, 2)
        out = np.zeros((len(rows), 2))
        margins = np.zeros(len(rows))
        lib().lyaref_sampler(seed, first, len(rows), _p(rows), _p(out),
                             _p(margins))
        return out, margins

    def trace(self, seed, first, n, max_events):
        out = np.zeros((n, HEADER + ROW * max_events))
        margins = np.zeros(n)
        lib().lyaref_trace(seed, first, n, _p(out), max_events, _p(margins))
        return out, margins

    def shoot(self, seed, first, n, statistics=False):
        """image (nx, ny), cube (nchan, nx, ny), unnormalised, the counters
        {steps, hydrogen, dust, rejections, deposits, capped, packets} and the
        run's smallest margin; with statistics also the sum of the squared
        addends to the cube and their number, (nchan, nx, ny) each"""
        s, m = self.s, self.s.m
        image = np.zeros((m.nx, m.ny))
        cube = np.zeros((s.nchan, m.nx, m.ny))
        squares = np.zeros((2, s.nchan, m.nx, m.ny)) if statistics else None
        c = (C.c_uint64 * 7)()
        margin = np.zeros(1)
        lib().lyaref_shoot(seed, first, n, _p(image), _p(cube),
                           None if squares is None else _p(squares), c,
                           _p(margin))
        counters = dict(zip(("nsteps", "nhydrogen", "ndust", "nrejections",
                             "natomics", "ncapped", "npackets"),
                            (int(v) for v in c)))
        if statistics:
            return image, cube, counters, float(margin[0]), squares[0], \
                squares[1]
        return image, cube, counters, float(margin[0])


def events(trace, max_events):
    """(rows [nrows][12] of all packets of a trace in order, the packet of
    each row)"""
    n = trace[:, 0].astype(int)
    assert n.max() <= max_events, n.max()
    rows = trace[:, HEADER:].reshape(len(trace), max_events, ROW)
    keep = np.arange(max_events)[None, :] < n[:, None]
    packet = np.broadcast_to(np.arange(len(trace))[:, None], keep.shape)
    return rows[keep], packet[keep]


# the scene of the parity tests: a 12^3 box of side 3e16 m with a density
# bump, a temperature gradient, an expanding velocity field and dust; the
# H I column gives a line-centre depth of a few hundred across the box, so
# that a packet scatters tens to hundreds of times
BOX_SIDE = 3.0e16
EXPANSION = 30.0e3  # m s^-1 at the box's face
# the packets whose traces the GPU is held to row by row, and the rows kept
# of each (test_lyman_alpha_host.py shows that none of them needs an excuse)
TRACE_SEED = 23
TRACE_PACKETS = 192
TRACE_EVENTS = 48


def cell_centres(model):
    return Q.cell_centres(model)


def parity_scene(ncell=(12, 12, 12), nchan=16, vmin=-2.0e5, vmax=2.0e5,
                 tau0=300., x_crit=0., albedo=0.5, dust_tau=0.5,
                 view=(1.1, 0.6), nx=12, ny=12, expansion=EXPANSION,
                 sigma_turb=0., dust=True, max_scatter=MAX_SCATTER):
    """see above; tau0 is the line-centre depth from the centre to a face at
    the mean density and 1e4 K, dust_tau the dust's over the same path"""
    import line_image_lib as LI
    half = 0.5 * BOX_SIDE
    box = LI.Box((-half, -half, -half), (BOX_SIDE,) * 3, ncell)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in ncell],
                               indexing="ij"), axis=-1).reshape(-1, 3)
    mid = (idx + 0.5) / np.array(ncell)
    x = (mid - 0.5) * BOX_SIDE
    r2 = (x * x).sum(axis=1) / half ** 2
    shape = 0.5 + np.exp(-2. * r2) + 0.2 * np.sin(5. * mid[:, 1])
    T = 8.0e3 + 6.0e3 * mid[:, 0] + 3.0e3 * mid[:, 2] ** 2
    sigma0 = line_centre_cross_section(doppler_width(1.0e4))
    n_HI = shape / shape.mean() * tau0 / (sigma0 * half)
    n_H = 1.0e4 * n_HI  # a neutral fraction of 1e-4
    sigma_d = dust_tau / (n_H.mean() * half)
    field = shape ** 2 * (r2 < 0.6)
    velocity = expansion * x / half if expansion else None
    theta, phi = view
    anchor, sides = LI.bounding_rectangle(box, theta, phi)
    model = SL.Model(box.anchor, box.sides, box.ncell, n_H, sigma_d, albedo,
                     0.44, 0.5, theta, phi, nx, ny, anchor, sides)
    return Scene(model, field, n_HI, T, nchan, vmin, vmax, velocity,
                 sigma_turb, x_crit, max_scatter, dust), box


# the physics anchor: a static uniform sphere of H I at 10 K inscribed in a
# 24^3 box, a tau_0 = 1000 from the centre to the edge, a source in the
# central cells, no dust
SPHERE_T = 10.
SPHERE_A_TAU0 = 1000.
SPHERE_X_CRIT = 3.
SPHERE_PACKETS = 4000
SPHERE_SEED = 3


def sphere_scene(ncell=24, nchan=1600):
    import line_image_lib as LI
    half = 0.5 * BOX_SIDE
    box = LI.Box((-half, -half, -half), (BOX_SIDE,) * 3, (ncell,) * 3)
    idx = np.stack(np.meshgrid(*[np.arange(ncell)] * 3, indexing="ij"),
                   axis=-1).reshape(-1, 3)
    x = ((idx + 0.5) / ncell - 0.5) * BOX_SIDE
    r = np.sqrt((x * x).sum(axis=1))
    b = float(doppler_width(SPHERE_T))
    a = float(voigt_parameter(b))
    tau0 = SPHERE_A_TAU0 / a
    n_HI = np.where(r <= half, tau0 / (line_centre_cross_section(b) * half),
                    0.)
    field = (r < 1.01 * np.sqrt(3.) * 0.5 * BOX_SIDE / ncell).astype(float)
    assert field.sum() == 8
    T = np.full(len(r), SPHERE_T)
    theta, phi = 0.9, 0.4
    anchor, sides = LI.bounding_rectangle(box, theta, phi)
    model = SL.Model(box.anchor, box.sides, box.ncell, np.maximum(n_HI, 1.),
                     0., 0., 0.44, 0.5, theta, phi, 8, 8, anchor, sides)
    vmax = 40. * b
    return Scene(model, field, n_HI, T, nchan, -vmax, vmax, None, 0.,
                 SPHERE_X_CRIT, dust=False), b, a


def sphere_statistics(cube, scene, b):
    """the median of |u| / b of the spectrum summed over the pixels, the blue
    share of its flux (u < 0 is blue: positive = receding), and the share of
    the flux in the cube of the image's"""
    from cmacionize_amd.engine import cube_channel_centres
    spectrum = cube.sum(axis=(1, 2))
    v = cube_channel_centres(scene.nchan, scene.vmin, scene.vmax)
    order = np.argsort(np.abs(v), kind="stable")
    c = np.cumsum(spectrum[order])
    median = float(np.abs(v)[order][np.searchsorted(c, 0.5 * c[-1])] / b)
    blue = float(spectrum[v < 0.].sum() / spectrum.sum())
    return median, blue
