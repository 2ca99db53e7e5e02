"""The CPU restatement of the escape tally (tests/support/escape_reference.c)
through ctypes - no GPU needed - and what the escape tests share: the numpy
form of the header's binning formula, the tilted frame, the test states."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "support", "escape_reference.c")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None

EV = 1.6021766208e-19 / 6.626070040e-34  # Hz per eV

# the pixel grid and bins of the parity tests
NLON, NMU = 12, 6
LINEAR_BINS = ("Linear", 8, 13.6 * EV, 54.4 * EV)
LEVEL_BINS = ("Level", 14, 0., 0.)
# no packet may come closer than this to a pixel edge (radians of l, units of
# mu) or a bin edge (relative): far above the last bits in which the device's
# atan2, sincos and log may differ from the host's
EDGE_MARGIN = 1e-9


def tilted_frame():
    """an orthonormal frame none of whose axes is a grid axis"""
    from cmacionize_amd.engine import sky_frame
    return sky_frame(pole=(0.3, -0.5, 0.8), zero_longitude=(0.9, 0.2, 0.1))


def lib():
    """Compile the restatement (gcc -O2 -ffp-contract=off -fopenmp, with the
    oracle's transport file inside it, linked against oracle/libcmio.so) once
    per version of its sources and load it."""
    global _lib
    if _lib is not None:
        return _lib
    O.build()
    digest = hashlib.sha256()
    for path in (SOURCE, os.path.join(O.ORACLE_DIR, "cmio_transport.c"),
                 os.path.join(O.ORACLE_DIR, "cmio_internal.h"),
                 os.path.join(O.ORACLE_DIR, "cmio.h")):
        digest.update(open(path, "rb").read())
    out = os.path.join(tempfile.gettempdir(), "cmi_escape_reference_%d_%s.so"
                       % (os.getuid(), digest.hexdigest()[:16]))
    if not os.path.exists(out):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off",
                        "-fopenmp", "-Wall", "-Wno-unused-function",
                        "-shared", "-fPIC", "-I", O.ORACLE_DIR, "-o", tmp,
                        SOURCE, "-L", O.ORACLE_DIR, "-lcmio",
                        "-Wl,-rpath," + O.ORACLE_DIR, "-lm"], check=True)
        os.replace(tmp, out)
    O.lib()  # (the oracle's error flag and its checked calls)
    lb = C.CDLL(out)
    lb.escref_shoot.argtypes = [
        C.POINTER(O.Grid), C.POINTER(O.Model), C.POINTER(O.Cells), C.c_uint32,
        C.c_uint32, C.c_uint64, C.c_uint64, _dp, _dp, _dp, C.c_int32,
        C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _dp, _dp]
    lb.escref_shoot.restype = None
    lb.escref_pixels.argtypes = [_dp, C.c_int32, C.c_int32, C.c_int64, _dp,
                                 _ip]
    lb.escref_pixels.restype = None
    _lib = lb
    return lb


def _p(a):
    return a.ctypes.data_as(_dp)


def shoot(sim, seed, iteration, first_packet, n_packets, nlon, nmu, frame,
          bins):
    """cmio_shoot's loop on an OracleSimulation with the tally: (tally (3,
    nfreq, nlon, nmu), totweight, typecount, (pixel edge distance, relative
    bin edge distance)). The simulation's integrals are added to as by
    sim.shoot."""
    kind, nfreq, fmin, fmax = bins
    if not sim.model.tables and (
            sim.model.spectrum_type == O.SPECTRUM_PLANCK or
            sim.model.reemit_type == O.REEMIT_PHYSICAL):
        sim.build_tables()
    f = np.ascontiguousarray(frame, dtype=np.float64).reshape(9)
    sky = np.zeros((3, nfreq, nlon, nmu))
    tw = C.c_double(0.)
    tc = np.zeros(O.NTYPE)
    edge = np.array([np.inf, np.inf])
    lib().escref_shoot(C.byref(sim.grid), C.byref(sim.model),
                       C.byref(sim.cells), seed, iteration, first_packet,
                       n_packets, C.byref(tw), _p(tc), _p(f), nlon, nmu,
                       nfreq, int(kind == "Level"), fmin, fmax, _p(sky),
                       _p(edge))
    return sky, tw.value, tc, (edge[0], edge[1])


def reference_pixels(directions, nlon, nmu, frame):
    d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(frame, dtype=np.float64).reshape(9)
    out = np.zeros(len(d), dtype=np.int32)
    lib().escref_pixels(_p(f), nlon, nmu, len(d), _p(d),
                        out.ctypes.data_as(_ip))
    return out


def numpy_pixels(directions, nlon, nmu, frame):
    """The header's formula in numpy: (pixel i * nmu + j, the distance of l
    (radians, the seam included) or mu (interior edges) to the nearest pixel
    edge)."""
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(frame, dtype=np.float64).reshape(3, 3)
    mu = d @ f[2]
    l = np.arctan2(d @ f[1], d @ f[0])
    fj = (mu + 1.) / 2. * nmu
    fi = (l + np.pi) / (2. * np.pi) * nlon
    j = np.clip(np.floor(fj).astype(np.int64), 0, nmu - 1)
    i = np.clip(np.floor(fi).astype(np.int64), 0, nlon - 1)
    l_edges = -np.pi + 2. * np.pi * np.arange(nlon + 1) / nlon
    dist = np.abs(l[:, None] - l_edges[None, :]).min(axis=1)
    if nmu > 1:
        mu_edges = -1. + 2. * np.arange(1, nmu) / nmu
        dist = np.minimum(dist,
                          np.abs(mu[:, None] - mu_edges[None, :]).min(axis=1))
    return i * nmu + j, dist


# the states of the parity tests -----------------------------------------------
LEX_NCELL, LEX_PACKETS, LEX_SEED = 20, 40000, 42

_lexington = None


def lexington_state():
    """lexington_simulation(20) after one iteration of 40000 packets with the
    temperature solve off: the OracleSimulation, made once and left as it is
    (shoot on a copy: lexington_copy)."""
    global _lexington
    if _lexington is None:
        sim = O.lexington_simulation(LEX_NCELL)
        sim.model.do_temperature = 0
        sim.run(LEX_PACKETS, 1, seed=LEX_SEED)
        _lexington = sim
    return _lexington


def lexington_copy():
    """a fresh simulation in lexington_state()'s cell state"""
    ref = lexington_state()
    sim = O.lexington_simulation(LEX_NCELL)
    sim.model.do_temperature = 0
    sim.number_density[:] = ref.number_density
    sim.temperature[:] = ref.temperature
    sim._xs[:] = ref._xs
    return sim


def lexington_engine(sim, **tuning):
    """a GpuEngine of the lexington model in the simulation's cell state"""
    from cmacionize_amd import GpuEngine, STROMGREN as S
    from test_oracle_physics import LEX
    eng = GpuEngine(sim.ncell, S["anchor"], S["sides"], (0, 0, 0), device=0,
                    track_heating=True)
    eng.set_sources([[0., 0., 0.]], [1.], 4.26e49)
    eng.set_spectrum_planck(40000.)
    eng.set_cross_sections_verner()
    eng.set_recombination_rates_verner()
    eng.set_abundances(LEX[1:])
    eng.set_reemission(1)
    eng.set_temperature_params(do_temperature_calculation=0,
                               pah_heating_factor=0.)
    eng.upload_cells(sim.number_density, sim.temperature,
                     np.array([np.asarray(x) for x in sim.x]))
    if tuning:
        eng.set_tuning(**tuning)
    return eng


PERIODIC_NCELL, PERIODIC_PACKETS, PERIODIC_SEED = 16, 40000, 9


def periodic_simulation():
    """The periodic Stromgren case: 16^3, x and y periodic, hydrogen only,
    diffuse re-emission, thin enough that packets cross the box more than
    once; a packet can leave through z only."""
    from cmacionize_amd import STROMGREN as S
    source = [[0.31 * S["sides"][0], -0.2 * S["sides"][0],
               0.07 * S["sides"][0]]]
    sim = O.OracleSimulation((PERIODIC_NCELL,) * 3, S["anchor"], S["sides"],
                             periodic=(1, 1, 0))
    sim.set_sources(source, [1.], S["luminosity"])
    sim.set_homogeneous(S["density"], S["temperature"], xH=2.e-5)
    m = sim.model
    m.spectrum_type = O.SPECTRUM_MONOCHROMATIC
    m.mono_frequency = S["frequency"]
    m.xsec_type = O.XSEC_FIXED
    m.xsec_fixed[0] = S["sigma_H"]
    m.recomb_type = O.RECOMB_FIXED
    m.recomb_fixed[0] = S["alpha_H"]
    m.reemit_type = O.REEMIT_PHYSICAL
    return sim, source


def periodic_engine(sim, source, **tuning):
    from cmacionize_amd import GpuEngine, STROMGREN as S
    eng = GpuEngine(sim.ncell, S["anchor"], S["sides"], (1, 1, 0), device=0,
                    track_heating=True)
    eng.set_sources(source, [1.], S["luminosity"])
    eng.set_spectrum_monochromatic(S["frequency"])
    sigma = np.zeros(14)
    sigma[0] = S["sigma_H"]
    alpha = np.zeros(14)
    alpha[0] = S["alpha_H"]
    eng.set_cross_sections_fixed(sigma)
    eng.set_recombination_rates_fixed(alpha)
    eng.set_reemission(1)
    eng.upload_cells(sim.number_density, sim.temperature,
                     np.array([np.asarray(x) for x in sim.x]))
    if tuning:
        eng.set_tuning(**tuning)
    return eng


_references = {}


def lexington_reference(bins):
    """The restatement's answer for the tally iteration of the lexington
    state (iteration 1, seed LEX_SEED, LEX_PACKETS packets, the tilted frame,
    NLON x NMU pixels): made once per kind of bins and left as it is."""
    if bins not in _references:
        _references[bins] = shoot(lexington_copy(), LEX_SEED, 1, 0,
                                  LEX_PACKETS, NLON, NMU, tilted_frame(),
                                  bins)
    return _references[bins]


def chi2_quantile(p, k):
    """The p quantile of the chi-square distribution with k degrees of
    freedom: the series of the regularised lower incomplete gamma function
    P(k / 2, x / 2) = p, solved by bisection."""
    import math
    a = 0.5 * k

    def cdf(x):
        z = 0.5 * x
        term = total = 1. / a
        n = 0
        while term > 1e-18 * total:
            n += 1
            term *= z / (a + n)
            total += term
        return total * math.exp(a * math.log(z) - z - math.lgamma(a))

    lo, hi = float(k), 20. * k
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if cdf(mid) < p:
            lo = mid
        else:
            hi = mid
    return hi
