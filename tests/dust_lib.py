"""The CPU restatement of the dusty radiative transfer mode
(tests/support/dust_reference.c) through ctypes, and the lowered parameters
of a dust parameter file as `cmi-gpu --dusty-radiative-transfer --dry-run
--describe` prints them (no GPU needed for either); make_engine sets the
same model up on the GPU engine."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "support", "dust_reference.c")
ORACLE = os.path.join(ROOT, "oracle")
CMI_GPU = os.path.join(ROOT, "cmacionize_amd", "cmi-gpu")
FIXTURES = os.path.join(HERE, "golden", "dust")

EMIT, SCATTER, SCATTER_TOWARDS, OPTICAL_DEPTH, TRACE = 0, 1, 2, 3, 4

_dp = C.POINTER(C.c_double)
_lib = None


def _p(a):
    return a.ctypes.data_as(_dp)


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp, linked
    against oracle/libcmio.so) once per source version and load it."""
    global _lib
    if _lib is not None:
        return _lib
    subprocess.run(["make", "-s", "-C", ORACLE], check=True)
    digest = hashlib.sha256(open(SOURCE, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(),
                       "cmi_dust_reference_%d_%s.so" % (os.getuid(), digest))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp",
                        "-Wall", "-shared", "-fPIC", "-o", tmp, SOURCE,
                        "-L" + ORACLE, "-lcmio", "-Wl,-rpath," + ORACLE,
                        "-lm"], check=True)
        os.replace(tmp, out)
    L = C.CDLL(out)
    i32p = C.POINTER(C.c_int32)
    L.dref_setup.argtypes = [_dp, _dp, i32p, _dp, _dp] + [C.c_double] * 6 + \
        [C.c_int32, C.c_int32, _dp, _dp] + [C.c_double] * 3
    L.dref_emit.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp]
    L.dref_scatter.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp, _dp]
    L.dref_scatter_towards.argtypes = [C.c_int64, _dp, _dp]
    L.dref_optical_depth.argtypes = [C.c_int64, _dp, _dp, C.c_int32]
    L.dref_trace.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp,
                             C.c_int32]
    L.dref_shoot.argtypes = [C.c_uint32, C.c_uint64, C.c_int64, _dp,
                             C.POINTER(C.c_uint64)]
    L.dref_pixel.restype = C.c_int64
    L.dref_pixel.argtypes = [_dp]
    L.dref_disc_cdf.argtypes = [_dp, _dp]
    L.dref_galaxy_density.argtypes = [_dp, _dp, i32p] + [C.c_double] * 3 + \
        [_dp]
    _lib = L
    return L


def describe(param_file, cwd):
    """The lowered values of a dust parameter file (JSON of --describe)."""
    r = subprocess.run([CMI_GPU, "--dusty-radiative-transfer", "--dry-run",
                        "--describe", "--params", param_file], cwd=cwd,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def galaxy_density(d):
    """number density (kg m^-3) per cell as the driver computes it"""
    n = int(np.prod(d["ncell"]))
    out = np.empty(n)
    lib().dref_galaxy_density(
        _p(np.array(d["anchor"], float)), _p(np.array(d["sides"], float)),
        np.array(d["ncell"], np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
        d["density"]["central_density"], d["density"]["scale_length_ISM"],
        d["density"]["scale_height_ISM"], _p(out))
    return out


class Restatement:
    """One model of the CPU restatement (module-wide state in the C code:
    the last Restatement set up is the one in use)."""

    def __init__(self, d, density, ncell=None):
        self.d = d
        self.ncell = list(ncell or d["ncell"])
        self.density = np.ascontiguousarray(density, dtype=float)
        self.xH = np.ones_like(self.density)
        self.setup()

    def setup(self):
        d = self.d
        img = d["image"]
        rc = lib().dref_setup(
            _p(np.array(d["anchor"], float)), _p(np.array(d["sides"], float)),
            np.array(self.ncell, np.int32).ctypes.data_as(
                C.POINTER(C.c_int32)),
            _p(self.density), _p(self.xH), d["dust"]["g"], d["dust"]["p_l"],
            d["dust"]["albedo"], d["dust"]["kappa"], img["theta"], img["phi"],
            img["width"], img["height"], _p(np.array(img["anchor"], float)),
            _p(np.array(img["sides"], float)),
            d["source"]["scale_length_stars"],
            d["source"]["scale_height_stars"],
            d["source"]["bulge_over_total"])
        assert rc == 0

    def emit(self, seed, first, n):
        out = np.zeros((n, 6))
        lib().dref_emit(seed, first, n, _p(out))
        return out

    def scatter(self, seed, first, rows):
        rows = np.ascontiguousarray(rows, dtype=float)
        out = np.zeros((len(rows), 12))
        lib().dref_scatter(seed, first, len(rows), _p(rows), _p(out))
        return out

    def scatter_towards(self, rows):
        rows = np.ascontiguousarray(rows, dtype=float)
        out = np.zeros((len(rows), 5))
        lib().dref_scatter_towards(len(rows), _p(rows), _p(out))
        return out

    def optical_depth(self, rows, max_cells):
        rows = np.ascontiguousarray(rows, dtype=float)
        out = np.zeros((len(rows), 2 + max_cells))
        lib().dref_optical_depth(len(rows), _p(rows), _p(out), max_cells)
        return out

    def trace(self, seed, first, n, max_events):
        out = np.zeros((n, 4 + 8 * max_events))
        lib().dref_trace(seed, first, n, _p(out), max_events)
        return out

    def shoot(self, seed, first, n):
        """image (3, nx, ny) of packets [first, first + n), counters
        {steps, scatterings, capped, dropped by the source}"""
        img = self.d["image"]
        image = np.zeros((3, img["width"], img["height"]))
        c = (C.c_uint64 * 4)()
        lib().dref_shoot(seed, first, n, _p(image), c)
        return image, [int(v) for v in c]

    def pixel(self, x):
        return int(lib().dref_pixel(_p(np.ascontiguousarray(x, float))))

    def disc_cdf(self):
        w = np.zeros(1001)
        p = np.zeros(1001)
        lib().dref_disc_cdf(_p(w), _p(p))
        return w, p


def make_engine(d, density):
    """a GpuEngine with the model `d` (describe()) and the given densities"""
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    eng = GpuEngine(d["ncell"], d["anchor"], d["sides"], (0, 0, 0), device=0)
    n = len(density)
    eng.upload_cells(np.ascontiguousarray(density, float), np.zeros(n), None)
    eng.upload_field(E.FIELD_IONIC_FRACTION + 0, np.ones(n))
    du, img, src = d["dust"], d["image"], d["source"]
    eng.set_dust_scattering(du["g"], du["p_l"], du["albedo"], du["kappa"])
    eng.set_ccd_image(img["theta"], img["phi"], img["width"], img["height"],
                      img["anchor"], img["sides"])
    eng.set_continuous_source_spiral_galaxy(
        src["scale_length_stars"], src["scale_height_stars"],
        src["bulge_over_total"])
    return eng
