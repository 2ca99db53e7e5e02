"""The CPU restatement of the scattered-light sky maps
(tests/support/scattered_sky_reference.c, which builds on
scattered_line_reference.c and dust_reference.c) through ctypes - no GPU
needed: the point camera of the dust mode on the device's random streams.
The model and the source are scattered_line_lib's; Camera holds what
cmi_gpu_set_sky_camera takes."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import scattered_line_lib as SL

SUPPORT = SL.SUPPORT
SOURCE = os.path.join(SUPPORT, "scattered_sky_reference.c")
SKY_PEEL = 6  # cmi_gpu_dust_probe kind
TRACE = 4
EINVAL, ESTATE = SL.EINVAL, SL.ESTATE

FULL_LON = (-np.pi, np.pi)
FULL_LAT = (-0.5 * np.pi, 0.5 * np.pi)
IDENTITY_FRAME = np.eye(3)

_dp = C.POINTER(C.c_double)
_lib = None
_p = SL._p
_f64 = SL._f64


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp, linked
    against oracle/libcmio.so) once per version of its three sources and
    load it."""
    global _lib
    if _lib is not None:
        return _lib
    subprocess.run(["make", "-s", "-C", SL.ORACLE], check=True)
    h = hashlib.sha256()
    for name in (SOURCE, SL.SOURCE, os.path.join(SUPPORT, "dust_reference.c")):
        h.update(open(name, "rb").read())
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_scattered_sky_reference_%d_%s.so" %
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
    L.slref_trace.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp,
                              C.c_int32]
    L.slref_trace.restype = None
    L.ssref_set_camera.argtypes = [_dp, _dp] + [C.c_double] * 4 + \
        [C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.ssref_set_camera.restype = None
    L.ssref_pixel.argtypes = [_dp]
    L.ssref_pixel.restype = C.c_int64
    L.ssref_peel.argtypes = [C.c_int64, _dp, _dp]
    L.ssref_peel.restype = None
    L.ssref_trace.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp,
                              C.c_int32]
    L.ssref_trace.restype = None
    L.ssref_shoot.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp, _dp,
                              _dp, C.POINTER(C.c_uint64)]
    L.ssref_shoot.restype = None
    _lib = L
    return L


def frame_of(pole=(0., 0., 1.), zero_longitude=(1., 0., 0.)):
    """rows e_1, e_2, e_3: the pole kept, the zero of longitude made
    perpendicular to it, e_2 = e_3 x e_1"""
    e3 = np.asarray(pole, dtype=float)
    e3 = e3 / np.sqrt(e3 @ e3)
    z = np.asarray(zero_longitude, dtype=float)
    e1 = z - (z @ e3) * e3
    e1 = e1 / np.sqrt(e1 @ e1)
    return np.array([e1, np.cross(e3, e1), e3])


class Camera:
    def __init__(self, origin, nlon, nlat, r_min, lon=FULL_LON, lat=FULL_LAT,
                 frame=IDENTITY_FRAME, direct_light=True):
        self.origin = _f64(origin).reshape(3)
        self.nlon, self.nlat = int(nlon), int(nlat)
        self.r_min = float(r_min)
        self.lon, self.lat = tuple(lon), tuple(lat)
        self.frame = _f64(frame).reshape(3, 3)
        self.direct_light = bool(direct_light)

    def solid_angles(self):
        """exact solid angles (nlon, nlat) of the pixels"""
        dl = (self.lon[1] - self.lon[0]) / self.nlon
        j = np.arange(self.nlat + 1)
        edges = self.lat[0] + (self.lat[1] - self.lat[0]) * j / self.nlat
        row = dl * np.diff(np.sin(edges))
        return np.broadcast_to(row, (self.nlon, self.nlat)).copy()

    def angles(self, positions):
        """longitude and latitude (radians) in which the observer sees the
        positions, and their distances"""
        v = np.asarray(positions, dtype=float) - self.origin
        r = np.sqrt((v * v).sum(axis=-1))
        n = v / r[..., None]
        e1, e2, e3 = self.frame
        return (np.arctan2(n @ e2, n @ e1),
                np.arcsin(np.clip(n @ e3, -1., 1.)), r)

    def apply(self, engine):
        engine.set_sky_camera(self.origin, self.nlon, self.nlat, self.r_min,
                              self.lon, self.lat, self.frame,
                              self.direct_light)


class Restatement:
    """One model, source field and camera of the CPU restatement
    (module-wide state in the C code: the last one set up is in use)."""

    def __init__(self, model, field, camera):
        self.m, self.cam = model, camera
        self.field = _f64(field).reshape(model.n)
        self.setup()

    def setup(self):
        m, k = self.m, self.cam
        ones = np.ones(m.n)
        L = lib()
        rc = L.dref_setup(
            _p(m.anchor), _p(m.sides),
            m.ncell.ctypes.data_as(C.POINTER(C.c_int32)), _p(m.density),
            _p(ones), m.g, m.p_l, m.albedo, m.sigma, m.theta, m.phi, m.nx,
            m.ny, _p(m.img_anchor), _p(m.img_sides), 1., 1., 0.)
        assert rc == 0
        assert L.slref_set_field(_p(self.field), m.n) == 0
        f = _f64(k.frame).reshape(9)
        L.ssref_set_camera(_p(k.origin), _p(f), k.lon[0], k.lon[1], k.lat[0],
                           k.lat[1], k.nlon, k.nlat, k.r_min,
                           int(k.direct_light))

    def total(self):
        t = np.zeros(1)
        lib().slref_get_tables(_p(t), None, None)
        return float(t[0])

    def pixel(self, x):
        return int(lib().ssref_pixel(_p(_f64(x))))

    def peel(self, rows):
        rows = _f64(rows).reshape(-1, 15)
        out = np.zeros((len(rows), 9))
        lib().ssref_peel(len(rows), _p(rows), _p(out))
        return out

    def trace(self, seed, first, n, max_events):
        out = np.zeros((n, 4 + 8 * max_events))
        lib().ssref_trace(seed, first, n, _p(out), max_events)
        return out

    def parallel_trace(self, seed, first, n, max_events):
        """the same packets seen by the model's parallel camera"""
        out = np.zeros((n, 4 + 8 * max_events))
        lib().slref_trace(seed, first, n, _p(out), max_events)
        return out

    def shoot(self, seed, first, n, statistics=False):
        """image (3, nlon, nlat), unnormalised, and the counters {steps,
        scatterings, capped, dropped, excluded, outside}; with statistics
        also, per pixel, the sum of the squared contributions to I and their
        number"""
        k = self.cam
        image = np.zeros((3, k.nlon, k.nlat))
        c = (C.c_uint64 * 6)()
        if not statistics:
            lib().ssref_shoot(seed, first, n, _p(image), None, None, c)
            return image, [int(v) for v in c]
        squares = np.zeros((k.nlon, k.nlat))
        hits = np.zeros((k.nlon, k.nlat))
        lib().ssref_shoot(seed, first, n, _p(image), _p(squares), _p(hits), c)
        return image, [int(v) for v in c], squares, hits


def events(trace, max_events):
    """the rows [nrows][8] of all packets of a trace, in order (packets whose
    rows did not fit are refused)"""
    n = trace[:, 0].astype(int)
    assert n.max() <= max_events, n.max()
    rows = trace[:, 4:].reshape(len(trace), max_events, 8)
    keep = np.arange(max_events)[None, :] < n[:, None]
    return rows[keep]


def make_engine(model, field, camera):
    """scattered_line_lib.make_engine with the sky camera selected"""
    eng = SL.make_engine(model, field)
    camera.apply(eng)
    return eng


# the albedo-0 identity's setup (tests/test_scattered_sky_host.py says how the
# values were chosen); the GPU's end-to-end test uses it too
IDENTITY_OBSERVER = (0.3, 2.1, 3.2)
IDENTITY_MAP = (24, 12)
IDENTITY_PACKETS = SL.IDENTITY_PACKETS
IDENTITY_SEED = SL.IDENTITY_SEED


def identity_scene():
    """box, model (albedo 0), the masked source field, the 0/1 mask and the
    camera of the albedo-0 identity: r_min = the longest cell side; the field
    density^2 is 0 in every cell that has a point within r_min of the
    observer (its nearest point to the observer is nearer than r_min)"""
    box, model, field = SL.identity_model(albedo=0.)
    cell = model.sides / model.ncell
    r_min = float(cell.max())
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in model.ncell],
                               indexing="ij"), axis=-1).reshape(-1, 3)
    lo = model.anchor + idx * cell
    nearest = np.clip(np.array(IDENTITY_OBSERVER), lo, lo + cell)
    d = np.sqrt(((nearest - np.array(IDENTITY_OBSERVER)) ** 2).sum(axis=1))
    mask = (d > r_min).astype(float)
    camera = Camera(IDENTITY_OBSERVER, IDENTITY_MAP[0], IDENTITY_MAP[1], r_min)
    return box, model, field * mask, mask, camera


def subray_directions(camera, sub=8):
    """sub x sub directions per pixel, uniform in longitude and in sin
    (latitude): equal solid angles, so that a pixel is their plain mean;
    (nlon, nlat, sub * sub, 3)"""
    k = camera
    u = (np.arange(k.nlon * sub) + 0.5) / (k.nlon * sub)
    lon = k.lon[0] + (k.lon[1] - k.lon[0]) * u
    j = np.arange(k.nlat + 1)
    edges = np.sin(k.lat[0] + (k.lat[1] - k.lat[0]) * j / k.nlat)
    t = (np.arange(sub) + 0.5) / sub
    sinb = (edges[:-1, None] + (edges[1:] - edges[:-1])[:, None] * t).ravel()
    cosb = np.sqrt(1. - sinb * sinb)
    e1, e2, e3 = k.frame
    d = (cosb[None, :, None] * np.cos(lon)[:, None, None] * e1 +
         cosb[None, :, None] * np.sin(lon)[:, None, None] * e2 +
         sinb[None, :, None] * e3)
    d = d.reshape(k.nlon, sub, k.nlat, sub, 3).transpose(0, 2, 1, 3, 4)
    return d.reshape(k.nlon, k.nlat, sub * sub, 3)
