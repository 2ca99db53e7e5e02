"""The CPU restatement of the sky maps (tests/support/sky_image_reference.c)
through ctypes - no GPU needed - and helpers the sky map tests share: sets of
directions, the distance from a point to the wall of a box in numpy."""
import ctypes as C
import hashlib
import itertools
import os
import subprocess
import tempfile

import numpy as np

from line_image_lib import Box, _f64, _p  # noqa: F401 (Box is re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "support", "sky_image_reference.c")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp) once per
    source version and load it."""
    global _lib
    if _lib is not None:
        return _lib
    digest = hashlib.sha256(open(SOURCE, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_sky_image_reference_%d_%s.so" % (os.getuid(),
                                                             digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.sref_probe.argtypes = [_dp, _dp, _ip, _dp, C.c_int64, _dp, C.c_int32,
                             _dp]
    L.sref_probe.restype = None
    L.sref_render.argtypes = [_dp, _dp, _ip, _dp, C.c_int64, _dp, C.c_int32,
                              _dp, _dp, _dp]
    L.sref_render.restype = C.c_int64
    _lib = L
    return L


def probe(box, origin, directions, max_cells):
    """rows {t_start, t_out, steps, cells[max_cells], ds[max_cells]}"""
    o = _f64(origin).reshape(3)
    d = _f64(directions).reshape(-1, 3)
    out = np.zeros((len(d), 3 + 2 * max_cells))
    lib().sref_probe(*box._args(), _p(o), len(d), _p(d), max_cells, _p(out))
    return out


last_crossings = 0


def render(box, fields, origin, directions, extinction=None):
    """intensities (nfields, nrays) of the per-cell quantities
    fields[nfields][ncell], with extinction[ncell] (m^-1) if given"""
    global last_crossings
    fields = _f64(fields).reshape(-1, box.n)
    o = _f64(origin).reshape(3)
    d = _f64(directions).reshape(-1, 3)
    k = None if extinction is None else _f64(extinction).reshape(box.n)
    out = np.zeros((len(fields), len(d)))
    for first in range(0, len(fields), 64):
        part = np.ascontiguousarray(fields[first:first + 64])
        res = np.zeros((len(part), len(d)))
        last_crossings = lib().sref_render(
            *box._args(), _p(o), len(d), _p(d), len(part), _p(part),
            _p(k) if k is not None else None, _p(res))
        out[first:first + len(part)] = res
    return out


def random_directions(rng, n):
    """n unit vectors, uniform on the sphere"""
    d = rng.normal(size=(n, 3))
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


def special_directions():
    """the 6 axis directions, the 12 face diagonals and the 8 body diagonals:
    zero components, and ties on the cubic grids"""
    out = []
    for v in itertools.product((-1., 0., 1.), repeat=3):
        v = np.array(v)
        if v.any():
            out.append(v / np.sqrt((v * v).sum()))
    assert len(out) == 26
    return np.array(out)


def wall_distance(box, origin, directions):
    """Distance from origin (inside the box) to the box wall along each
    direction, in closed form: the smallest of (wall - o) / d over the axes,
    with the wall the ray looks at (divisions, not products with 1 / d)."""
    o = _f64(origin).reshape(3)
    d = _f64(directions).reshape(-1, 3)
    lo, hi = box.anchor, box.anchor + box.sides
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0., (hi - o) / d,
                     np.where(d < 0., (lo - o) / d, np.inf))
    return t.min(axis=1)
