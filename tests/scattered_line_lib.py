"""The CPU restatement of the scattered-light line images
(tests/support/scattered_line_reference.c, which builds on dust_reference.c)
through ctypes - no GPU needed: the cell-luminosity source's tables and
selection rule and the packet's life on the device's random streams;
make_engine sets the same model up on the GPU engine."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SUPPORT = os.path.join(HERE, "support")
SOURCE = os.path.join(SUPPORT, "scattered_line_reference.c")
ORACLE = os.path.join(ROOT, "oracle")
CMI_GPU = os.path.join(ROOT, "cmacionize_amd", "cmi-gpu")

BLOCK = 256  # CMI_CELL_SOURCE_BLOCK
CELL_SOURCE = 5  # cmi_gpu_dust_probe kind
EINVAL, ESTATE = 1, 3  # include/cmi_gpu.h

_dp = C.POINTER(C.c_double)
_lib = None


def _p(a):
    return a.ctypes.data_as(_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp, linked
    against oracle/libcmio.so) once per version of its two sources and load
    it."""
    global _lib
    if _lib is not None:
        return _lib
    subprocess.run(["make", "-s", "-C", ORACLE], check=True)
    h = hashlib.sha256()
    for name in (SOURCE, os.path.join(SUPPORT, "dust_reference.c")):
        h.update(open(name, "rb").read())
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_scattered_line_reference_%d_%s.so" %
                       (os.getuid(), h.hexdigest()[:16]))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                        "-o", tmp, SOURCE, "-L" + ORACLE, "-lcmio",
                        "-Wl,-rpath," + ORACLE, "-lm"], check=True)
        os.replace(tmp, out)
    L = C.CDLL(out)
    i32p = C.POINTER(C.c_int32)
    i64p = C.POINTER(C.c_int64)
    L.dref_setup.argtypes = [_dp, _dp, i32p, _dp, _dp] + [C.c_double] * 6 + \
        [C.c_int32, C.c_int32, _dp, _dp] + [C.c_double] * 3
    L.dref_pixel.restype = C.c_int64
    L.dref_pixel.argtypes = [_dp]
    L.slref_set_field.argtypes = [_dp, C.c_int64]
    L.slref_get_tables.argtypes = [_dp, _dp, _dp]
    L.slref_get_tables.restype = None
    L.slref_select.argtypes = [C.c_int64, _dp, i64p]
    L.slref_select.restype = None
    L.slref_emit.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp]
    L.slref_emit.restype = None
    L.slref_trace.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp,
                              C.c_int32]
    L.slref_trace.restype = None
    L.slref_shoot.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp, _dp,
                              _dp, C.POINTER(C.c_uint64)]
    L.slref_shoot.restype = None
    _lib = L
    return L


class Model:
    """What a run needs besides the source: the grid (anchor[3], sides[3],
    ncell[3]), the gas density (m^-3 per cell), the dust (cross section per
    hydrogen nucleus sigma, albedo, g, p_l) and the image (theta, phi, nx,
    ny, anchor[2], sides[2])."""

    def __init__(self, anchor, sides, ncell, density, sigma, albedo, g, p_l,
                 theta, phi, nx, ny, img_anchor, img_sides):
        self.anchor = _f64(anchor).reshape(3)
        self.sides = _f64(sides).reshape(3)
        self.ncell = np.ascontiguousarray(ncell, dtype=np.int32).reshape(3)
        self.n = int(np.prod(self.ncell.astype(np.int64)))
        self.density = _f64(density).reshape(self.n)
        self.sigma, self.albedo, self.g, self.p_l = sigma, albedo, g, p_l
        self.theta, self.phi, self.nx, self.ny = theta, phi, int(nx), int(ny)
        self.img_anchor = _f64(img_anchor).reshape(2)
        self.img_sides = _f64(img_sides).reshape(2)

    @property
    def pixel_area(self):
        return self.img_sides[0] * self.img_sides[1] / (self.nx * self.ny)

    def describe(self):
        """the dictionary test_gpu_dust.py's helpers read"""
        return {"anchor": list(self.anchor), "sides": list(self.sides),
                "ncell": [int(v) for v in self.ncell],
                "image": {"theta": self.theta, "phi": self.phi,
                          "width": self.nx, "height": self.ny,
                          "anchor": list(self.img_anchor),
                          "sides": list(self.img_sides)}}


class Restatement:
    """One model and one source field of the CPU restatement (module-wide
    state in the C code: the last one set up is the one in use)."""

    def __init__(self, model, field):
        self.m = model
        self.field = _f64(field).reshape(model.n)
        self.status = None
        self.setup()

    def setup(self):
        m = self.m
        ones = np.ones(m.n)
        rc = lib().dref_setup(
            _p(m.anchor), _p(m.sides),
            m.ncell.ctypes.data_as(C.POINTER(C.c_int32)), _p(m.density),
            _p(ones), m.g, m.p_l, m.albedo, m.sigma, m.theta, m.phi, m.nx,
            m.ny, _p(m.img_anchor), _p(m.img_sides), 1., 1., 0.)
        assert rc == 0
        self.status = lib().slref_set_field(_p(self.field), m.n)
        return self.status

    def tables(self):
        """total luminosity (W), block sums B, cell sums C"""
        nblock = (self.m.n + BLOCK - 1) // BLOCK
        total = np.zeros(1)
        B = np.zeros(nblock)
        Cs = np.zeros(self.m.n)
        lib().slref_get_tables(_p(total), _p(B), _p(Cs))
        return float(total[0]), B, Cs

    def select(self, u):
        u = _f64(u).ravel()
        cells = np.zeros(len(u), dtype=np.int64)
        lib().slref_select(len(u), _p(u),
                           cells.ctypes.data_as(C.POINTER(C.c_int64)))
        return cells

    def emit(self, seed, first, n):
        out = np.zeros((n, 7))
        lib().slref_emit(seed, first, n, _p(out))
        return out

    def trace(self, seed, first, n, max_events):
        out = np.zeros((n, 4 + 8 * max_events))
        lib().slref_trace(seed, first, n, _p(out), max_events)
        return out

    def shoot(self, seed, first, n, statistics=False):
        """image (3, nx, ny) of packets [first, first + n), unnormalised, and
        the counters {steps, scatterings, capped, dropped}; with statistics
        also, per pixel, the sum of the squared contributions to I and
        their number"""
        m = self.m
        image = np.zeros((3, m.nx, m.ny))
        c = (C.c_uint64 * 4)()
        if not statistics:
            lib().slref_shoot(seed, first, n, _p(image), None, None, c)
            return image, [int(v) for v in c]
        squares = np.zeros((m.nx, m.ny))
        hits = np.zeros((m.nx, m.ny))
        lib().slref_shoot(seed, first, n, _p(image), _p(squares), _p(hits), c)
        return image, [int(v) for v in c], squares, hits

    def pixel(self, x):
        return int(lib().dref_pixel(_p(_f64(x))))


def make_engine(model, field=None):
    """a GpuEngine with `model`'s grid, gas, dust and image; `field` (if
    given) as its cell source"""
    from cmacionize_amd import GpuEngine
    m = model
    eng = GpuEngine(tuple(int(v) for v in m.ncell), tuple(m.anchor),
                    tuple(m.sides), (0, 0, 0), device=0)
    eng.upload_cells(m.density, np.zeros(m.n), None)
    eng.set_dust_scattering_per_hydrogen(m.g, m.p_l, m.albedo, m.sigma)
    eng.set_ccd_image(m.theta, m.phi, m.nx, m.ny, m.img_anchor, m.img_sides)
    if field is not None:
        eng.set_cell_source_field(field)
    return eng


def fields():
    """{name: (ncell[3], weights)}: the shapes the tables are tested on,
    integer-valued weights (every sum is exact): one partial block; four
    full blocks and one of 56; blocks 1 and 2 dark; a single emitting cell"""
    rng = np.random.default_rng(5)
    out = {}
    out["4x4x4"] = ((4, 4, 4), rng.integers(0, 9, 64).astype(float))
    w = rng.integers(0, 1000, 1080).astype(float)
    w[rng.uniform(size=1080) < 0.3] = 0.
    out["10x12x9"] = ((10, 12, 9), w)
    w = rng.integers(0, 50, 1080).astype(float)
    w[BLOCK:3 * BLOCK] = 0.
    out["blocks 1 and 2 dark"] = ((10, 12, 9), w)
    w = np.zeros(1080)
    w[777] = 3.
    out["one cell"] = ((10, 12, 9), w)
    return out


def unit_model(ncell, sigma=0.):
    """a unit box of unit density with a small image, for tests of the
    source alone"""
    n = int(np.prod(ncell))
    return Model((0., 0., 0.), (1., 1., 1.), ncell, np.ones(n), sigma, 0.5,
                 0.4, 0.3, 0.7, 0.3, 8, 8, (-1., -1.), (2., 2.))


# the statistical identity's setup (tests/test_scattered_line_host.py says
# how the values were chosen); the GPU's end-to-end test uses it too
IDENTITY_NCELL = (10, 12, 9)
IDENTITY_VIEW = (1.1, 0.6)
IDENTITY_SIGMA = 0.08  # x density ~ 1 per unit length: tau ~ 1 over the box
IDENTITY_PACKETS = 400000
IDENTITY_SEED = 11


def identity_model(albedo=0., nx=16, ny=16):
    """the 10 x 12 x 9 grid of the statistical identity: a box of sides
    (2.5, 3, 2.25), a smooth density of 5 .. 20, an emissivity proportional
    to its square, a 16 x 16 image over the box's bounding rectangle"""
    import line_image_lib as L
    box = L.Box((-1., 0.5, 2.), (2.5, 3., 2.25), IDENTITY_NCELL)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in IDENTITY_NCELL],
                               indexing="ij"), axis=-1).reshape(-1, 3)
    mid = (idx + 0.5) / np.array(IDENTITY_NCELL)
    density = 5. + 10. * mid[:, 0] + 5. * np.sin(3. * mid[:, 1]) ** 2
    # (what a recombination line of gas at one temperature and ionisation
    # emits, up to a factor)
    field = density ** 2
    theta, phi = IDENTITY_VIEW
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    model = Model(box.anchor, box.sides, box.ncell, density, IDENTITY_SIGMA,
                  albedo, 0.44, 0.5, theta, phi, nx, ny, anchor, sides)
    return box, model, field
