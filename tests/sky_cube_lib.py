"""The CPU restatement of the sky cubes (tests/support/sky_cube_reference.c)
through ctypes - no GPU needed - and what the sky cube tests share: a numpy
transcription of the contract for a handful of rays, the channel block, the
radial velocities of a ray list."""
import ctypes as C
import hashlib
import math
import os
import re
import subprocess
import tempfile

import numpy as np

import sky_image_lib as S
from sky_image_lib import Box, _f64, _p  # noqa: F401 (Box is re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "support", "sky_cube_reference.c")

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
                       "cmi_sky_cube_reference_%d_%s.so" % (os.getuid(),
                                                            digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    lb = C.CDLL(out)
    lb.scref_render.argtypes = [_dp, _dp, _ip, _dp, _dp, C.c_int64, _dp,
                                C.c_int32, _dp, _dp, _dp, _dp, C.c_int32,
                                C.c_double, C.c_double, _dp]
    lb.scref_render.restype = C.c_int64
    _lib = lb
    return lb


last_crossings = 0


def render(box, fields, widths, origin, directions, nchan, vmin, vmax,
           extinction=None, velocity=None, observer_velocity=None):
    """cube (nfields, nchan, nrays) of the per-cell sources
    fields[nfields][ncell] with the widths[nfields][ncell]"""
    global last_crossings
    fields = _f64(fields).reshape(-1, box.n)
    widths = _f64(widths).reshape(len(fields), box.n)
    o = _f64(origin).reshape(3)
    d = _f64(directions).reshape(-1, 3)
    k = None if extinction is None else _f64(extinction).reshape(box.n)
    v = None if velocity is None else _f64(velocity).reshape(3, box.n)
    vo = (None if observer_velocity is None
          else _f64(observer_velocity).reshape(3))
    out = np.zeros((len(fields), nchan, len(d)))
    last_crossings = lib().scref_render(
        *box._args(), _p(o), _p(vo) if vo is not None else None, len(d),
        _p(d), len(fields), _p(fields), _p(widths),
        _p(k) if k is not None else None, _p(v) if v is not None else None,
        nchan, vmin, vmax, _p(out))
    return out


def edges(nchan, vmin, vmax):
    dv = (vmax - vmin) / nchan
    return vmin + np.arange(nchan + 1) * dv


def radial_velocity(w, d):
    """(w_x d_x + w_y d_y) + w_z d_z in the contract's order; w (3,) or
    (3, ncell), d (nrays, 3): (nrays,) or (nrays, ncell)"""
    w = np.asarray(w, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    if w.ndim == 1:
        return (w[0] * d[:, 0] + w[1] * d[:, 1]) + w[2] * d[:, 2]
    return ((w[0][None] * d[:, :1] + w[1][None] * d[:, 1:2]) +
            w[2][None] * d[:, 2:])


def transcription(box, fields, widths, origin, directions, nchan, vmin, vmax,
                  extinction=None, velocity=None, observer_velocity=None):
    """The contract in numpy scalars over the cells and path lengths of the
    sky maps' restatement (its probe rows): slow, for a handful of rays."""
    fields = _f64(fields).reshape(-1, box.n)
    widths = _f64(widths).reshape(len(fields), box.n)
    d = _f64(directions).reshape(-1, 3)
    nmax = int(box.ncell.sum()) + 3
    rows = S.probe(box, origin, d, nmax)
    e = edges(nchan, vmin, vmax)
    vo = np.zeros(3) if observer_velocity is None else _f64(observer_velocity)
    vel = (np.zeros((3, box.n)) if velocity is None
           else _f64(velocity).reshape(3, box.n))
    w = vel - vo.reshape(3, 1)
    out = np.zeros((len(fields), nchan, len(d)))

    def E(x, u, b):
        if b == 0.:
            return 1. if x - u > 0. else -1.
        z = (x - u) / b
        return 1. if z >= 6. else (-1. if z <= -6. else math.erf(z))

    for r in range(len(d)):
        steps = int(rows[r, 2])
        cells = rows[r, 3:3 + steps].astype(int)
        ds = rows[r, 3 + nmax:3 + nmax + steps]
        for l in range(len(fields)):
            T = 1.
            I = np.zeros(nchan)
            for cell, s in zip(cells, ds):
                u = ((w[0, cell] * d[r, 0] + w[1, cell] * d[r, 1]) +
                     w[2, cell] * d[r, 2])
                k = 0. if extinction is None else extinction[cell]
                q = fields[l, cell] / (4. * np.pi)
                if k == 0.:
                    emitted, att = q * s, 1.
                else:
                    dtau = k * s
                    emitted = (q / k) * -math.expm1(-dtau)
                    att = math.exp(-dtau)
                Es = [E(x, u, widths[l, cell]) for x in e]
                for c in range(nchan):
                    I[c] += T * (emitted * (0.5 * (Es[c + 1] - Es[c])))
                T = T * att
            out[l, :, r] = I
    return out


def channel_block():
    """CB, the channels per march launch (sky_cube_kernels.h)"""
    text = open(os.path.join(ROOT, "cmacionize_amd", "csrc",
                             "sky_cube_kernels.h")).read()
    return int(re.search(r"#define CMI_SKY_CUBE_CB (\d+)", text).group(1))
