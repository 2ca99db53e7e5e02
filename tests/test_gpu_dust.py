"""GPU tests of the dusty radiative transfer mode (cmi_gpu_dust_*, dust
kernels in cmacionize_amd/csrc/device_dust.h / dust_kernels.h) against the
CPU restatement tests/support/dust_reference.c on the same random streams,
and the driver `cmi-gpu --dusty-radiative-transfer` end to end.

Tolerances. Both sides run the same IEEE sequence (-ffp-contract=off on both)
except for the transcendentals: the device's sin / cos / exp / log / pow /
acos / atan2 (ROCm's OCML) and glibc's differ by an ulp or two. Positions,
Stokes vectors and weights therefore agree to ~1e-15 relative per
operation; a few hundred operations along a trace keep that below 1e-12. The
exceptions are arc cosines near +-1 (phi' = phi +- acos(cos dphi) in
DustScattering::scatter): there d acos / dx = 1 / sqrt(1 - x^2) turns an ulp
into up to ~1e-8 rad, so directions after a scattering are compared at 1e-7.
The DDA's cell sequences involve no transcendental and must be identical.
"""
import os
import subprocess

import numpy as np
import pytest

import dust_lib

pytestmark = pytest.mark.gpu

FIX = dust_lib.FIXTURES
GALAXY = os.path.join(FIX, "dusty_galaxy.param")
TEST32 = os.path.join(FIX, "test_dustsimulation.param")
SEED = 42


@pytest.fixture(scope="module")
def d32(tmp_path_factory):
    return dust_lib.describe(TEST32, str(tmp_path_factory.mktemp("d32")))


make_engine = dust_lib.make_engine


@pytest.fixture(scope="module")
def galaxy32(d32):
    density = dust_lib.galaxy_density(d32)
    assert density.max() > 0.
    eng = make_engine(d32, density)
    ref = dust_lib.Restatement(d32, density)
    yield d32, eng, ref
    eng.close()


# ------------------------------------------------------------ probes --

def test_emission_positions(galaxy32):
    d, eng, ref = galaxy32
    ref.setup()
    n = 20000
    gpu = eng.dust_probe(dust_lib.EMIT, SEED, 0, n)
    cpu = ref.emit(SEED, 0, n)
    side = d["sides"][0]
    # positions: a cos / sin / log and a few products each
    assert np.allclose(gpu[:, 0:3], cpu[:, 0:3], rtol=0., atol=1e-13 * side)
    assert np.allclose(gpu[:, 3:6], cpu[:, 3:6], rtol=0., atol=1e-15)
    lo = np.array(d["anchor"])
    assert np.all(gpu[:, 0:3] >= lo) and np.all(gpu[:, 0:3] < lo + side)


def _rows(n, seed, polarised):
    rng = np.random.default_rng(seed)
    cost = rng.uniform(-1., 1., n)
    phi = rng.uniform(0., 2. * np.pi, n)
    sint = np.sqrt(1. - cost ** 2)
    rows = np.zeros((n, 12))
    rows[:, 0:3] = np.stack([sint * np.cos(phi), sint * np.sin(phi), cost], 1)
    rows[:, 3:8] = np.stack([sint, cost, phi, np.sin(phi), np.cos(phi)], 1)
    rows[:, 8] = 1.
    if polarised:
        q = rng.uniform(-0.4, 0.4, (n, 3))
        rows[:, 9:12] = q
        rows[:, 8:12] *= rng.uniform(0.1, 2., (n, 1))
    # both |cos| == 1 branches: photons along the z axis
    rows[0, 0:8] = [0., 0., 1., 0., 1., 0., 0., 1.]
    rows[1, 0:8] = [0., 0., -1., 0., -1., 0., 0., 1.]
    return rows


@pytest.mark.parametrize("polarised", [False, True])
def test_scatter(galaxy32, polarised):
    d, eng, ref = galaxy32
    ref.setup()
    rows = _rows(20000, 5, polarised)
    gpu = eng.dust_probe(dust_lib.SCATTER, 9, 0, len(rows), rows)
    cpu = ref.scatter(9, 0, rows)
    # direction and its angles: acos near +-1 (see the module docstring)
    assert np.allclose(gpu[:, 0:8], cpu[:, 0:8], rtol=0., atol=1e-7)
    close = np.all(np.abs(gpu[:, 0:8] - cpu[:, 0:8]) <= 1e-12, axis=1)
    assert close.mean() > 0.999
    # Stokes: pow / acos / cos / exp of the same angle
    I = np.abs(cpu[:, 8:9])
    assert np.allclose(gpu[:, 8:12], cpu[:, 8:12], rtol=0., atol=1e-12 * I)


@pytest.mark.parametrize("polarised", [False, True])
def test_scatter_towards(galaxy32, polarised):
    d, eng, ref = galaxy32
    ref.setup()
    rows = _rows(20000, 6, polarised)
    gpu = eng.dust_probe(dust_lib.SCATTER_TOWARDS, 0, 0, len(rows), rows)
    cpu = ref.scatter_towards(rows)
    assert np.allclose(gpu[:, 0], cpu[:, 0], rtol=1e-13, atol=0.)
    I = np.abs(cpu[:, 1:2])
    assert np.allclose(gpu[:, 1:5], cpu[:, 1:5], rtol=0., atol=1e-12 * I)


def test_optical_depth_and_cell_sequences(galaxy32):
    d, eng, ref = galaxy32
    ref.setup()
    n, cap = 4000, 128
    start = ref.emit(SEED, 0, n)
    rows = start.copy()
    # half of the rays towards the observer
    img = d["image"]
    obs = [np.sin(img["theta"]) * np.cos(img["phi"]),
           np.sin(img["theta"]) * np.sin(img["phi"]), np.cos(img["theta"])]
    rows[::2, 3:6] = obs
    gpu = eng.dust_probe(dust_lib.OPTICAL_DEPTH, 0, 0, n, rows, cap)
    cpu = ref.optical_depth(rows, cap)
    assert np.array_equal(gpu[:, 1], cpu[:, 1])      # steps
    assert np.array_equal(gpu[:, 2:], cpu[:, 2:])    # the cells, in order
    # no transcendental: the same sums
    assert np.array_equal(gpu[:, 0], cpu[:, 0])
    assert cpu[:, 0].max() > 0.1


def test_traces(galaxy32):
    d, eng, ref = galaxy32
    ref.setup()
    n, cap = 2000, 64
    gpu = eng.dust_probe(dust_lib.TRACE, SEED, 0, n, None, cap)
    cpu = ref.trace(SEED, 0, n, cap)
    assert np.all(gpu[:, 3] == 0.)
    assert cpu[:, 1].max() >= 2  # some packets scatter more than once
    side = d["sides"][0]
    ev = np.minimum(np.minimum(cpu[:, 0], gpu[:, 0]), cap).astype(int)
    g = gpu[:, 4:].reshape(n, cap, 8)
    c = cpu[:, 4:].reshape(n, cap, 8)
    # a packet whose number of events differs: its traces agree up to a
    # flight that ends, on one side, on the box's face - the optical depth
    # drawn equals the one to the edge to rounding (the forced first
    # interaction draws tau <= tau_max: u near 1 puts it on the face)
    for k in np.flatnonzero(gpu[:, 0] != cpu[:, 0]):
        longer = g[k] if gpu[k, 0] > cpu[k, 0] else c[k]
        assert ev[k] < cap
        assert _on_box_face(d, longer[ev[k], 0:3]), (k, gpu[k, :4],
                                                     cpu[k, :4])
    for k in range(n):
        a, b = g[k, :ev[k]], c[k, :ev[k]]
        assert np.allclose(a[:, 0:3], b[:, 0:3], rtol=0., atol=1e-12 * side), k
        assert np.allclose(a[:, 3:7], b[:, 3:7], rtol=0.,
                           atol=1e-11 * np.abs(b[:, 3:4])), k
        assert np.allclose(a[:, 7], b[:, 7], rtol=1e-11, atol=0.), k


def _on_box_face(d, x, tol=1e-9):
    """x lies on a face of the box, to tol of the box side"""
    lo = np.array(d["anchor"])
    hi = lo + np.array(d["sides"])
    return np.min(np.minimum(np.abs(x - lo), np.abs(hi - x)) /
                  np.array(d["sides"])) < tol


# ---------------------------------------------------------- whole runs --

def test_zero_density_only_direct_light(d32):
    n = int(np.prod(d32["ncell"]))
    eng = make_engine(d32, np.zeros(n))
    ref = dust_lib.Restatement(d32, np.zeros(n))
    N = 50000
    eng.dust_shoot(SEED, 0, N)
    image = eng.download_image()
    c = eng.get_dust_counters()
    eng.close()
    assert c["npackets"] == N and c["nscatter"] == 0 and c["ncapped"] == 0
    assert np.all(image[1] == 0.) and np.all(image[2] == 0.)
    pos = ref.emit(SEED, 0, N)[:, 0:3]
    hist = np.zeros(image[0].size)
    for x in pos:
        p = ref.pixel(x)
        if p >= 0:
            hist[p] += 0.25 / np.pi
    # equal addends: every order of the additions gives the same sums
    assert np.array_equal(image[0].ravel(), hist)
    assert hist.sum() > 0.


def test_source_box_must_contain_the_origin(d32):
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    d = d32
    anchor = list(d["anchor"])
    anchor[2] = 20. * 3.086e19
    eng = GpuEngine(d["ncell"], anchor, d["sides"], (0, 0, 0), device=0)
    src = d["source"]
    with pytest.raises(E.EngineError) as info:
        eng.set_continuous_source_spiral_galaxy(
            src["scale_length_stars"], src["scale_height_stars"],
            src["bulge_over_total"])
    assert "origin" in str(info.value)
    # and without a source nothing is shot
    with pytest.raises(E.EngineError):
        eng.dust_shoot(SEED, 0, 10)
    eng.close()


def test_source_gives_up_after_a_million_attempts(d32):
    """A box around the origin too small for the source: every packet's
    rejection loop ends after 1e6 attempts, is counted, and the image is
    refused as incomplete."""
    from cmacionize_amd import engine as E
    d = dict(d32)
    d["anchor"] = [-0.001 * 3.086e19] * 3
    d["sides"] = [0.002 * 3.086e19] * 3
    d["ncell"] = [4, 4, 4]
    eng = make_engine(d, np.zeros(64))
    out = eng.dust_probe(dust_lib.EMIT, SEED, 0, 4)
    assert np.all(np.isnan(out))
    eng.dust_shoot(SEED, 0, 64)
    c = eng.get_dust_counters()
    assert c["nsource_capped"] == 64 and c["npackets"] == 64
    assert c["nsteps"] == 0
    with pytest.raises(E.EngineError) as info:
        eng.download_image()
    assert "no position" in str(info.value)
    eng.close()


def _bad_pixels(gpu, cpu):
    """pixels where the GPU image differs from the restatement's by more
    than rtol 1e-9 (Q and U are signed sums: near-cancelled pixels are
    compared at 1e-12 of the image's largest |I|)"""
    atol = 1e-12 * np.abs(cpu[0]).max()
    return ~np.isclose(gpu, cpu, rtol=1e-9, atol=atol)


def _culprits(eng, ref, lo, hi, mask, out):
    """packets in [lo, hi) whose contributions differ on the masked pixels:
    images are additive over packet ranges, so halve the range"""
    eng.reset_image()
    eng.dust_shoot(SEED, lo, hi - lo)
    gpu = eng.download_image()
    cpu, _ = ref.shoot(SEED, lo, hi - lo)
    if not np.any(_bad_pixels(gpu, cpu) & mask):
        return
    if hi - lo == 1:
        out.append(lo)
        return
    mid = (lo + hi) // 2
    _culprits(eng, ref, lo, mid, mask, out)
    _culprits(eng, ref, mid, hi, mask, out)


def _is_threshold_case(d, ref, gpu_tr, cpu_tr, cap):
    """the trace of a culprit: the first event whose pixel differs between
    the two sides sits on a pixel edge (to 1e-9 of a pixel), or the number of
    events differs where one side's flight ended on the box's face or a
    position lies on a cell wall (to 1e-9)"""
    img = d["image"]
    g = gpu_tr[4:].reshape(cap, 8)
    c = cpu_tr[4:].reshape(cap, 8)
    n = int(min(gpu_tr[0], cpu_tr[0], cap))
    st, ct = np.sin(img["theta"]), np.cos(img["theta"])
    sp, cp = np.sin(img["phi"]), np.cos(img["phi"])
    for k in range(n):
        if ref.pixel(g[k, :3]) != ref.pixel(c[k, :3]):
            x = c[k, :3]
            u = (x[1] * cp - x[0] * sp - img["anchor"][0]) / img["sides"][0] \
                * img["width"]
            v = (x[2] * st - x[1] * ct * sp - x[0] * ct * cp -
                 img["anchor"][1]) / img["sides"][1] * img["height"]
            return min(abs(u - round(u)), abs(v - round(v))) < 1e-9
    if gpu_tr[0] != cpu_tr[0]:
        longer = g if gpu_tr[0] > cpu_tr[0] else c
        if n < cap and _on_box_face(d, longer[n, 0:3]):
            return True
        cell = np.array(d["sides"]) / np.array(d["ncell"])
        for k in range(n):
            f = (c[k, :3] - np.array(d["anchor"])) / cell
            if np.min(np.abs(f - np.round(f))) < 1e-9:
                return True
        return False
    return False


def test_whole_run_32(galaxy32):
    d, eng, ref = galaxy32
    ref.setup()
    N = 50000
    eng.reset_image()
    eng.dust_shoot(SEED, 0, N)
    gpu = eng.download_image()
    c = eng.get_dust_counters()
    cpu, cc = ref.shoot(SEED, 0, N)
    assert c["npackets"] == N and c["ncapped"] == 0 and cc[2] == 0
    assert c["nsource_capped"] == 0 and cc[3] == 0
    assert np.count_nonzero(cpu[0]) > 1000
    bad = _bad_pixels(gpu, cpu)
    if not np.any(bad):
        assert c["nscatter"] == cc[1]
        assert c["nsteps"] == cc[0]
    else:
        culprits = []
        _culprits(eng, ref, 0, N, bad, culprits)
        assert culprits, "differing pixels without a differing packet"
        cap = 4096
        for k in culprits:
            gt = eng.dust_probe(dust_lib.TRACE, SEED, k, 1, None, cap)[0]
            ct = ref.trace(SEED, k, 1, cap)[0]
            assert _is_threshold_case(d, ref, gt, ct, cap), k
        # every pixel the culprits do not touch agrees
        eng.reset_image()
        ok = np.ones(N, bool)
        ok[culprits] = False
        gpu2 = np.zeros_like(gpu)
        cpu2 = np.zeros_like(cpu)
        edges = np.flatnonzero(np.diff(np.r_[0, ok.astype(int), 0]))
        for lo, hi in zip(edges[0::2], edges[1::2]):
            eng.reset_image()
            eng.dust_shoot(SEED, int(lo), int(hi - lo))
            gpu2 += eng.download_image()
            cpu2 += ref.shoot(SEED, int(lo), int(hi - lo))[0]
        assert not np.any(_bad_pixels(gpu2, cpu2))


def test_additive_and_deterministic(galaxy32):
    d, eng, ref = galaxy32
    N, a = 30000, 12345
    eng.reset_image()
    eng.dust_shoot(SEED, 0, N)
    whole = eng.download_image()
    eng.reset_image()
    eng.dust_shoot(SEED, 0, a)
    eng.dust_shoot(SEED, a, N - a)
    parts = eng.download_image()
    c = eng.get_dust_counters()
    assert c["ncapped"] == 0 and c["npackets"] == N
    # the same terms, added in another order by the atomics
    atol = 1e-14 * np.abs(whole[0]).max()
    assert np.allclose(parts, whole, rtol=1e-12, atol=atol)


# ------------------------------------------------------------- driver --

def _variant(tmp_path, replace):
    text = open(GALAXY).read()
    for old, new in replace:
        assert old in text
        text = text.replace(old, new)
    p = tmp_path / "galaxy.param"
    p.write_text(text)
    return str(p)


def test_driver_end_to_end_201(tmp_path):
    r = subprocess.run([dust_lib.CMI_GPU, "--dusty-radiative-transfer",
                        "--params", GALAXY, "--device", "0"],
                       cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Total photon shooting time" in r.stdout
    assert (tmp_path / "dust-parameters-usedvalues.param").exists()
    dat = tmp_path / "galaxy_image.dat"
    assert dat.stat().st_size == 320000
    image = np.fromfile(str(dat), dtype=np.float64).reshape(200, 200)
    (tmp_path / "describe").mkdir()
    d = dust_lib.describe(GALAXY, str(tmp_path / "describe"))
    N = d["number_of_photons"]
    eng = make_engine(d, dust_lib.galaxy_density(d))
    eng.dust_shoot(d["random_seed"], 0, N)
    abi = eng.download_image()[0] * (1. / N)
    eng.close()
    assert abi.max() > 0.
    assert np.allclose(image, abi, rtol=1e-12, atol=1e-15 * abi.max())

    pgm = tmp_path / "pgm"
    pgm.mkdir()
    p = _variant(pgm, [("type: BinaryArray", "type: PGM"),
                       ("number of photons: 500000",
                        "number of photons: 20000")])
    r = subprocess.run([dust_lib.CMI_GPU, "--dusty-radiative-transfer",
                        "--params", p], cwd=str(pgm), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = (pgm / "galaxy_image.pgm").read_text().split("\n")
    assert lines[0:3] == ["P2", "200 200", "255"]
    values = np.array([[int(v) for v in l.split()] for l in lines[3:203]])
    assert values.shape == (200, 200)
    assert values.min() == 0 and values.max() == 255
