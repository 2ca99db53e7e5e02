"""The CPU restatement of the spectral line cubes
(tests/support/line_cube_reference.c) through ctypes - no GPU needed - and
what the cube tests share: the analytic channel fractions, the test box and
its views."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import tempfile

import numpy as np

import line_image_lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "support", "line_cube_reference.c")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None
_p, _f64 = L._p, L._f64

# the shapes every cube test uses: an offset anchor, unequal sides, images
# with a margin (some rays miss), axis-aligned and oblique views
BOX = L.Box((-1., 0.5, 2.), (3., 2., 2.5), (12, 10, 9))
NX, NY = 23, 17
HALF = 0.5 * np.pi
VIEWS = [(0., 0.), (HALF, 0.), (HALF, HALF), (0.7, 0.3), (2.1, 4.0),
         (np.radians(89.7), 0.4)]


def image_rectangle(box, theta, phi, margin=0.1):
    """the bounding rectangle of the box with a margin on every side"""
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    return anchor - margin * sides, (1. + 2. * margin) * sides


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp) once per
    source version and load it."""
    global _lib
    if _lib is not None:
        return _lib
    digest = hashlib.sha256(open(SOURCE, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_line_cube_reference_%d_%s.so" % (os.getuid(),
                                                             digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    lb = C.CDLL(out)
    lb.cref_render.argtypes = [_dp, _dp, _ip, C.c_double, C.c_double,
                               C.c_int32, C.c_int32, _dp, _dp, C.c_int32,
                               C.c_int32, _dp, _dp, _dp, _dp, C.c_int32,
                               C.c_double, C.c_double, _dp]
    lb.cref_render.restype = C.c_int64
    _lib = lb
    return lb


last_crossings = 0


def render(box, fields, widths, theta, phi, nx, ny, anchor, sides, nchan,
           vmin, vmax, supersample=1, extinction=None, velocity=None):
    """cube (nfields, nchan, nx, ny) of the per-cell sources fields[nfields]
    [ncell] with the widths[nfields][ncell]"""
    global last_crossings
    fields = _f64(fields).reshape(-1, box.n)
    widths = _f64(widths).reshape(len(fields), box.n)
    a = _f64(anchor).reshape(2)
    s = _f64(sides).reshape(2)
    k = None if extinction is None else _f64(extinction).reshape(box.n)
    v = None if velocity is None else _f64(velocity).reshape(3, box.n)
    out = np.zeros((len(fields), nchan, nx, ny))
    last_crossings = lib().cref_render(
        *box._args(), theta, phi, nx, ny, _p(a), _p(s), supersample,
        len(fields), _p(fields), _p(widths),
        _p(k) if k is not None else None, _p(v) if v is not None else None,
        nchan, vmin, vmax, _p(out))
    return out


def edges(nchan, vmin, vmax):
    dv = (vmax - vmin) / nchan
    return vmin + np.arange(nchan + 1) * dv


def fractions(nchan, vmin, vmax, u, b):
    """the channel fractions of a line at u with width b > 0, from math.erf
    (no clamp: erf is 1 to the last bit where the contract clamps)"""
    e = np.array([math.erf((x - u) / b) for x in edges(nchan, vmin, vmax)])
    return 0.5 * (e[1:] - e[:-1])


def longest_ray(box, theta, phi, nx, ny, anchor, sides, s=1):
    xy = L.sample_coordinates(nx, ny, anchor, sides, s).reshape(-1, 2)
    return int(L.probe(box, theta, phi, xy, 0)[:, 2].max())


def channel_block():
    """CB, the channels per march launch (line_cube_kernels.h)"""
    import re
    text = open(os.path.join(L.ROOT, "cmacionize_amd", "csrc",
                             "line_cube_kernels.h")).read()
    return int(re.search(r"#define CMI_LINE_CUBE_CB (\d+)", text).group(1))
