"""The CPU restatement of the emission-line images
(tests/support/line_image_reference.c) through ctypes - no GPU needed - and
helpers the line image tests share: the bounding rectangle of a box under a
view, an independent slab test in numpy."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "support", "line_image_reference.c")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None


def _p(a):
    return a.ctypes.data_as(_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp) once per
    source version and load it."""
    global _lib
    if _lib is not None:
        return _lib
    digest = hashlib.sha256(open(SOURCE, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_line_image_reference_%d_%s.so" % (os.getuid(),
                                                              digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.lref_probe.argtypes = [_dp, _dp, _ip, C.c_double, C.c_double,
                             C.c_int64, _dp, C.c_int32, _dp]
    L.lref_probe.restype = None
    L.lref_render.argtypes = [_dp, _dp, _ip, C.c_double, C.c_double,
                              C.c_int32, C.c_int32, _dp, _dp, C.c_int32,
                              C.c_int32, _dp, _dp, _dp]
    L.lref_render.restype = C.c_int64
    _lib = L
    return L


class Box:
    """A box with its grid: anchor[3], sides[3], ncell[3]."""

    def __init__(self, anchor, sides, ncell):
        self.anchor = _f64(anchor).reshape(3)
        self.sides = _f64(sides).reshape(3)
        self.ncell = np.ascontiguousarray(ncell, dtype=np.int32).reshape(3)
        self.n = int(np.prod(self.ncell.astype(np.int64)))

    @property
    def cellside(self):
        return self.sides / self.ncell

    def _args(self):
        return _p(self.anchor), _p(self.sides), self.ncell.ctypes.data_as(_ip)


def probe(box, theta, phi, xy, max_cells):
    """rows {t_in, t_out, steps, cells[max_cells], ds[max_cells]}"""
    xy = _f64(xy).reshape(-1, 2)
    out = np.zeros((len(xy), 3 + 2 * max_cells))
    lib().lref_probe(*box._args(), theta, phi, len(xy), _p(xy), max_cells,
                     _p(out))
    return out


last_crossings = 0


def render(box, fields, theta, phi, nx, ny, anchor, sides, supersample=1,
           extinction=None):
    """images (nfields, nx, ny) of the per-cell quantities fields[nfields]
    [ncell], with extinction[ncell] (m^-1) if given"""
    global last_crossings
    fields = _f64(fields).reshape(-1, box.n)
    a = _f64(anchor).reshape(2)
    s = _f64(sides).reshape(2)
    k = None if extinction is None else _f64(extinction).reshape(box.n)
    out = np.zeros((len(fields), nx, ny))
    last_crossings = 0
    for first in range(0, len(fields), 64):
        part = np.ascontiguousarray(fields[first:first + 64])
        img = np.zeros((len(part), nx, ny))
        last_crossings = lib().lref_render(
            *box._args(), theta, phi, nx, ny, _p(a), _p(s), supersample,
            len(part), _p(part), _p(k) if k is not None else None, _p(img))
        out[first:first + len(part)] = img
    return out


def axes(theta, phi):
    """n, e_x, e_y of a view"""
    st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    return (np.array([st * cp, st * sp, ct]), np.array([-sp, cp, 0.]),
            np.array([-ct * cp, -ct * sp, st]))


def bounding_rectangle(box, theta, phi):
    """anchor[2], sides[2] of the rectangle around the box's eight projected
    corners"""
    _, ex, ey = axes(theta, phi)
    corners = np.array([[box.anchor[a] + ((c >> a) & 1) * box.sides[a]
                         for a in range(3)] for c in range(8)])
    px, py = corners @ ex, corners @ ey
    lo = np.array([px.min(), py.min()])
    hi = np.array([px.max(), py.max()])
    return lo, hi - lo


def chords(box, theta, phi, xy):
    """Length of each ray inside the box, by a slab test of its own (numpy,
    divisions instead of the products with 1 / n); 0 for a miss."""
    n, ex, ey = axes(theta, phi)
    xy = _f64(xy).reshape(-1, 2)
    o = xy[:, :1] * ex[None, :] + xy[:, 1:] * ey[None, :]
    tin = np.full(len(xy), -np.inf)
    tout = np.full(len(xy), np.inf)
    hit = np.ones(len(xy), dtype=bool)
    for a in range(3):
        lo, hi = box.anchor[a], box.anchor[a] + box.sides[a]
        if n[a] != 0.:
            t0, t1 = (lo - o[:, a]) / n[a], (hi - o[:, a]) / n[a]
            tin = np.maximum(tin, np.minimum(t0, t1))
            tout = np.minimum(tout, np.maximum(t0, t1))
        else:
            hit &= (o[:, a] >= lo) & (o[:, a] < hi)
    return np.where(hit & (tout > tin), tout - tin, 0.)


def sample_coordinates(nx, ny, anchor, sides, supersample=1):
    """image coordinates of every sample: (nx, ny, s, s, 2)"""
    s = supersample
    fx = (np.arange(nx)[:, None] + (np.arange(s)[None, :] + 0.5) / s) / nx
    fy = (np.arange(ny)[:, None] + (np.arange(s)[None, :] + 0.5) / s) / ny
    x = anchor[0] + sides[0] * fx
    y = anchor[1] + sides[1] * fy
    out = np.empty((nx, ny, s, s, 2))
    out[..., 0] = x[:, None, :, None]
    out[..., 1] = y[None, :, None, :]
    return out
