"""The CPU restatement of the scattered-light line cubes
(tests/support/scattered_cube_reference.c, which builds on
scattered_sky_reference.c, scattered_line_reference.c and dust_reference.c)
through ctypes - no GPU needed: the Doppler bookkeeping of a packet and the
channel shares of its events, on the walk and the random streams of the
scattered-light images. The model and the source are scattered_line_lib's, the
point camera scattered_sky_lib's; Cube holds what cmi_gpu_set_scattered_cube
takes."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import scattered_line_lib as SL
import scattered_sky_lib as SS

SUPPORT = SL.SUPPORT
SOURCE = os.path.join(SUPPORT, "scattered_cube_reference.c")
CUBE_TRACE = 7  # cmi_gpu_dust_probe kind
EINVAL, ESTATE = SL.EINVAL, SL.ESTATE
BOLTZMANN = 1.38064852e-23
ATOMIC_MASS_UNIT = 1.660539040e-27
HYDROGEN = 1.00794  # cmi_emission_atomic_weight of HAlpha

_dp = C.POINTER(C.c_double)
_lib = None
_p = SL._p
_f64 = SL._f64


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp, linked
    against oracle/libcmio.so) once per version of its four sources and load
    it."""
    global _lib
    if _lib is not None:
        return _lib
    subprocess.run(["make", "-s", "-C", SL.ORACLE], check=True)
    h = hashlib.sha256()
    for name in (SOURCE, SS.SOURCE, SL.SOURCE,
                 os.path.join(SUPPORT, "dust_reference.c")):
        h.update(open(name, "rb").read())
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_scattered_cube_reference_%d_%s.so" %
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
    L.dref_setup.argtypes = [_dp, _dp, i32p, _dp, _dp] + [C.c_double] * 6 + \
        [C.c_int32, C.c_int32, _dp, _dp] + [C.c_double] * 3
    L.slref_set_field.argtypes = [_dp, C.c_int64]
    L.slref_get_tables.argtypes = [_dp, _dp, _dp]
    L.slref_get_tables.restype = None
    L.ssref_set_camera.argtypes = [_dp, _dp] + [C.c_double] * 4 + \
        [C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.ssref_set_camera.restype = None
    L.scube_set_cube.argtypes = [C.c_int32] + [C.c_double] * 3 + \
        [_dp, _dp, C.c_double, _dp, _dp]
    L.scube_set_cube.restype = None
    L.scube_shares.argtypes = [C.c_double, C.c_double, _dp]
    L.scube_shares.restype = None
    L.scube_trace.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_int64,
                              _dp, C.c_int32]
    L.scube_trace.restype = None
    L.scube_shoot.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_int64,
                              _dp, _dp, _dp, C.POINTER(C.c_uint64)]
    L.scube_shoot.restype = None
    _lib = L
    return L


class Cube:
    """The arguments of cube mode: the channel axis, sigma_turb, the widths b
    per cell (a field source), the cell velocities (ncell, 3) or None, the
    observer's velocity or None"""

    def __init__(self, nchan, vmin, vmax, widths, sigma_turb=0.,
                 velocity=None, observer_velocity=None):
        self.nchan, self.vmin, self.vmax = int(nchan), float(vmin), float(vmax)
        self.sigma_turb = float(sigma_turb)
        self.widths = _f64(widths).ravel()
        self.velocity = None if velocity is None else \
            _f64(_f64(velocity).reshape(-1, 3).T)  # [3][ncell]
        self.observer_velocity = None if observer_velocity is None else \
            _f64(observer_velocity).reshape(3)

    def apply(self, engine):
        """on an engine whose camera and field source are set"""
        engine.set_cell_velocities(self.velocity)
        engine.set_scattered_cube(self.nchan, self.vmin, self.vmax,
                                  self.sigma_turb, widths=self.widths,
                                  observer_velocities=self.observer_velocity)


class Restatement:
    """One model, source field, cube and (for the point camera) camera of the
    CPU restatement (module-wide state in the C code: the last one set up is
    in use)."""

    def __init__(self, model, field, cube, camera=None):
        self.m, self.cube, self.cam = model, cube, camera
        self.field = _f64(field).reshape(model.n)
        self.setup()

    @property
    def point(self):
        return int(self.cam is not None)

    @property
    def shape(self):
        return (self.cam.nlon, self.cam.nlat) if self.cam is not None else \
            (self.m.nx, self.m.ny)

    def setup(self):
        m, k, q = self.m, self.cam, self.cube
        ones = np.ones(m.n)
        L = lib()
        rc = L.dref_setup(
            _p(m.anchor), _p(m.sides),
            m.ncell.ctypes.data_as(C.POINTER(C.c_int32)), _p(m.density),
            _p(ones), m.g, m.p_l, m.albedo, m.sigma, m.theta, m.phi, m.nx,
            m.ny, _p(m.img_anchor), _p(m.img_sides), 1., 1., 0.)
        assert rc == 0
        assert L.slref_set_field(_p(self.field), m.n) == 0
        if k is not None:
            f = _f64(k.frame).reshape(9)
            L.ssref_set_camera(_p(k.origin), _p(f), k.lon[0], k.lon[1],
                               k.lat[0], k.lat[1], k.nlon, k.nlat, k.r_min,
                               int(k.direct_light))
        L.scube_set_cube(
            q.nchan, q.vmin, q.vmax, q.sigma_turb, _p(q.widths), None, 0.,
            None if q.velocity is None else _p(q.velocity),
            None if q.observer_velocity is None else _p(q.observer_velocity))

    def shares(self, u, b):
        f = np.zeros(self.cube.nchan)
        lib().scube_shares(u, b, _p(f))
        return f

    def trace(self, seed, first, n, max_events):
        out = np.zeros((n, 4 + 10 * max_events))
        lib().scube_trace(self.point, seed, first, n, _p(out), max_events)
        return out

    def shoot(self, seed, first, n, statistics=False):
        """image (3, nx, ny), cube (3, nchan, nx, ny), unnormalised, and the
        counters {steps, scatterings, capped, excluded, outside, events that
        reached a pixel}; with statistics also the sum of the squared addends
        to the cube's I and their number, (nchan, nx, ny) each"""
        shape = self.shape
        image = np.zeros((3,) + shape)
        cube = np.zeros((3, self.cube.nchan) + shape)
        squares = np.zeros((2, self.cube.nchan) + shape) if statistics \
            else None
        c = (C.c_uint64 * 6)()
        lib().scube_shoot(self.point, seed, first, n, _p(image), _p(cube),
                          None if squares is None else _p(squares), c)
        counters = [int(v) for v in c]
        if statistics:
            return image, cube, counters, squares[0], squares[1]
        return image, cube, counters


def events(trace, max_events):
    """the rows [nrows][10] of all packets of a trace, in order"""
    n = trace[:, 0].astype(int)
    assert n.max() <= max_events, n.max()
    rows = trace[:, 4:].reshape(len(trace), max_events, 10)
    keep = np.arange(max_events)[None, :] < n[:, None]
    return rows[keep]


def cell_centres(model):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in model.ncell],
                               indexing="ij"), axis=-1).reshape(-1, 3)
    return model.anchor + (idx + 0.5) * (model.sides / model.ncell)


# the scene of the trace tests: a velocity field linear in position (a shear)
# plus solid rotation about z through the box's centre, km/s scale
SHEAR = np.array([[3.0e3, -1.0e3, 0.5e3],
                  [0.7e3, -2.0e3, 1.5e3],
                  [-1.2e3, 0.4e3, 2.5e3]])  # s^-1 x m: dv_i / dx_j
OMEGA = 4.0e3  # m s^-1 per m
TRACE_SIGMA_TURB = 2.0e3
TRACE_SEED = 23


def trace_velocity(model):
    """(ncell, 3) velocities of the trace scene, and its largest speed and
    the norm of its gradient (m s^-1 per m)"""
    x = cell_centres(model) - (model.anchor + 0.5 * model.sides)
    v = x @ SHEAR.T
    v[:, 0] += -OMEGA * x[:, 1]
    v[:, 1] += OMEGA * x[:, 0]
    grad = SHEAR + OMEGA * np.array([[0., -1., 0.], [1., 0., 0.],
                                     [0., 0., 0.]])
    return v, float(np.sqrt((v * v).sum(axis=1)).max()), \
        float(np.linalg.norm(grad, 2))


def trace_widths(model):
    """b per cell of the trace scene: 8 to 12 km/s, smooth"""
    x = (cell_centres(model) - model.anchor) / model.sides
    return 8.0e3 + 4.0e3 * x[:, 0] * x[:, 2]


def near_wall(model, positions, tol=1e-9):
    """positions that lie within tol cell sides of a cell wall"""
    f = (np.asarray(positions) - model.anchor) / (model.sides / model.ncell)
    return np.min(np.abs(f - np.round(f)), axis=-1) < tol
