"""CPU tests of the dusty radiative transfer mode: the fixture files, the
driver's lowering of them (`cmi-gpu --dusty-radiative-transfer --dry-run
--describe`), its errors, and invariants of the CPU restatement
(tests/support/dust_reference.c) that the GPU tests compare the device path
against."""
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import stats

import dust_lib

FIX = dust_lib.FIXTURES
GALAXY = os.path.join(FIX, "dusty_galaxy.param")
TEST32 = os.path.join(FIX, "test_dustsimulation.param")
KPC = 3.086e19


def test_fixtures_match_their_sums():
    lines = open(os.path.join(FIX, "SHA256SUMS")).read().split("\n")
    sums = dict(reversed(l.split()) for l in lines if l.strip())
    assert sorted(sums) == ["dusty_galaxy.param", "test_dustsimulation.param"]
    for name, digest in sums.items():
        data = open(os.path.join(FIX, name), "rb").read()
        assert hashlib.sha256(data).hexdigest() == digest, name


@pytest.mark.parametrize("fixture,ncell,nphoton", [
    (GALAXY, 201, 500000), (TEST32, 32, 50000)])
def test_describe_lowers_the_fixture(tmp_path, fixture, ncell, nphoton):
    d = dust_lib.describe(fixture, str(tmp_path))
    assert d["mode"] == "dusty-radiative-transfer"
    assert d["ncell"] == [ncell] * 3
    assert d["number_of_photons"] == nphoton
    assert d["random_seed"] == 42
    assert d["anchor"] == pytest.approx([-12. * KPC] * 3, rel=1e-15)
    assert d["sides"] == pytest.approx([24. * KPC] * 3, rel=1e-15)
    # DustScattering, band V (src/DustScattering.hpp:62-160)
    assert d["dust"] == {"band": "V", "g": 0.44, "p_l": 0.43, "albedo": 0.54,
                         "kappa": 21.9}
    # B/T corrected for the bulge's cut-off centre:
    # 0.2 (1 - (rC / (rC + rJ)) / (rB / (rB + rJ)))
    rC, rB, rJ = 0.2 * KPC, 2. * KPC, 0.4 * KPC
    src = d["source"]
    assert src["bulge_over_total"] == 0.2
    assert src["bulge_over_total_corrected"] == pytest.approx(
        0.2 * (1. - (rC / (rC + rJ)) / (rB / (rB + rJ))), rel=1e-15)
    assert src["bulge_over_total_corrected"] == pytest.approx(0.12,
                                                              rel=1e-12)
    assert src["scale_length_stars"] == pytest.approx(5. * KPC, rel=1e-15)
    assert src["scale_height_stars"] == pytest.approx(0.6 * KPC, rel=1e-15)
    # n_0 = 1 cm^-3 = 1e6 m^-3, times 1.674e-27 (a mass density)
    dens = d["density"]
    assert dens["central_density"] == pytest.approx(1.674e-27 * 1e6,
                                                    rel=1e-15)
    assert dens["scale_length_ISM"] == pytest.approx(6. * KPC, rel=1e-15)
    assert dens["scale_height_ISM"] == pytest.approx(0.22 * KPC, rel=1e-15)
    img = d["image"]
    assert img["anchor"] == pytest.approx([-12.1 * KPC] * 2, rel=1e-15)
    assert img["sides"] == pytest.approx([24.2 * KPC] * 2, rel=1e-15)
    assert img["theta"] == pytest.approx(math.radians(89.7), rel=1e-15)
    assert img["phi"] == 0.
    assert (img["width"], img["height"]) == (200, 200)
    assert img["type"] == "BinaryArray"
    # the used values go next to the output, as in the reference
    assert (tmp_path / "dust-parameters-usedvalues.param").exists()


def _variant(tmp_path, source, replace):
    text = open(source).read()
    for old, new in replace:
        assert old in text
        text = text.replace(old, new)
    path = tmp_path / "variant.param"
    path.write_text(text)
    return str(path)


def test_band_K(tmp_path):
    p = _variant(tmp_path, TEST32, [("band: V", "band: K")])
    d = dust_lib.describe(p, str(tmp_path))
    assert d["dust"] == {"band": "K", "g": 0.02, "p_l": 0.93, "albedo": 0.21,
                         "kappa": 2.}


@pytest.mark.parametrize("replace,message", [
    ([("band: V", "band: B")], "Unknown band: B"),
    ([("type: BinaryArray", "type: FITS")], "Unknown image type: FITS"),
    ([("sides: [24. kpc, 24. kpc, 24. kpc]",
       "sides: [24. kpc, 24. kpc, 24. kpc]\n  periodicity: [true, false, "
       "false]")], "Periodic boxes are not supported"),
    # the spiral galaxy source is centred on the origin
    ([("anchor: [-12. kpc, -12. kpc, -12. kpc]",
       "anchor: [-12. kpc, -12. kpc, 20. kpc]")], "must contain the origin"),
])
def test_errors(tmp_path, replace, message):
    p = _variant(tmp_path, TEST32, replace)
    r = subprocess.run([dust_lib.CMI_GPU, "--dusty-radiative-transfer",
                        "--dry-run", "--describe", "--params", p],
                       cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stderr


def test_usage_names_the_mode():
    r = subprocess.run([dust_lib.CMI_GPU, "--no-such-flag"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--dusty-radiative-transfer" in r.stderr


# ------------------------------------------------ the CPU restatement --

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = dust_lib.describe(TEST32, str(tmp_path_factory.mktemp("describe")))
    return d


def _restatement(d, **source):
    d = dict(d)
    d["source"] = dict(d["source"], **source)
    n = int(np.prod(d["ncell"]))
    return dust_lib.Restatement(d, np.zeros(n))


def _photon_rows(rng, n, stokes=(1., 0., 0., 0.)):
    """random directions with their angles, given Stokes vector"""
    cost = rng.uniform(-1., 1., n)
    phi = rng.uniform(0., 2. * np.pi, n)
    sint = np.sqrt(1. - cost ** 2)
    rows = np.zeros((n, 12))
    rows[:, 0] = sint * np.cos(phi)
    rows[:, 1] = sint * np.sin(phi)
    rows[:, 2] = cost
    rows[:, 3] = sint
    rows[:, 4] = cost
    rows[:, 5] = phi
    rows[:, 6] = np.sin(phi)
    rows[:, 7] = np.cos(phi)
    rows[:, 8:12] = stokes
    return rows


def test_hg_sampling_mean_cosine_is_g(model):
    ref = _restatement(model)
    rows = _photon_rows(np.random.default_rng(1), 200000)
    out = ref.scatter(7, 0, rows)
    mu = np.sum(rows[:, 0:3] * out[:, 0:3], axis=1)
    g = model["dust"]["g"]
    # the HG variance is 1/3 (1 + 2 g^2) - g^2
    sigma = math.sqrt((1. + 2. * g * g) / 3. - g * g) / math.sqrt(len(mu))
    assert abs(mu.mean() - g) < 5. * sigma
    # new directions are unit vectors, and consistent with their angles
    assert np.allclose(np.sum(out[:, 0:3] ** 2, axis=1), 1., atol=1e-12)
    assert np.allclose(out[:, 2], out[:, 4], atol=0.)
    assert np.allclose(out[:, 0], out[:, 3] * out[:, 7], atol=1e-15)


def test_peel_off_phase_function_is_normalised(model):
    """4 pi <hgfac> over isotropic directions (relative to the observer) is
    1: the HG phase function per steradian integrates to one."""
    ref = _restatement(model)
    rows = _photon_rows(np.random.default_rng(2), 400000)
    out = ref.scatter_towards(rows)
    est = 4. * np.pi * out[:, 0].mean()
    # relative standard error of the estimate
    err = out[:, 0].std() / out[:, 0].mean() / math.sqrt(len(out))
    assert abs(est - 1.) < 5. * err


def test_unpolarised_light_keeps_I_and_polarises_at_most_p_l(model):
    ref = _restatement(model)
    rows = _photon_rows(np.random.default_rng(3), 50000)
    pl = model["dust"]["p_l"]
    for out, cols in ((ref.scatter(11, 0, rows), slice(8, 12)),
                      (ref.scatter_towards(rows), slice(1, 5))):
        I, Q, U, V = out[:, cols].T
        assert np.allclose(I, 1., rtol=0., atol=4e-16)
        dop = np.sqrt(Q * Q + U * U) / I
        assert dop.max() <= pl * (1. + 1e-12)
        assert dop.max() > 0.9 * pl  # and it does polarise
        assert np.all(V == 0.) or np.abs(V).max() < 1e-15


def test_stokes_vectors_stay_physical_over_50_scatterings(model):
    ref = _restatement(model)
    rows = _photon_rows(np.random.default_rng(4), 2000)
    for k in range(50):
        out = ref.scatter(5, 1000000 * k, rows)
        rows = out.copy()
        I, Q, U, V = rows[:, 8:12].T
        assert np.all(I * I * (1. + 1e-12) >= Q * Q + U * U + V * V), k
        assert np.all(I > 0.)


def test_source_radii_and_heights(model):
    """Disc only (B/T = 0) in a box large enough that the rejection loop
    drops almost nothing: cylindrical radii follow 1 - (1 + x) e^-x with
    x = w / r_stars, |z| is exponential with scale h_stars."""
    d = dict(model)
    d["anchor"] = [-60. * KPC] * 3
    d["sides"] = [120. * KPC] * 3
    ref = _restatement(d, bulge_over_total=0.)
    pos = ref.emit(42, 0, 20000)[:, 0:3]
    rs = model["source"]["scale_length_stars"]
    hs = model["source"]["scale_height_stars"]
    w = np.hypot(pos[:, 0], pos[:, 1]) / rs
    assert stats.kstest(w, lambda x: 1. - (1. + x) * np.exp(-x)).pvalue > 1e-3
    z = np.abs(pos[:, 2]) / hs
    assert stats.kstest(z, "expon").pvalue > 1e-3
    # and the z signs are balanced
    assert abs(np.mean(pos[:, 2] > 0.) - 0.5) < 0.02
    # the CDF table of the constructor: 1001 points to 1.2 |anchor|
    x, y = ref.disc_cdf()
    assert x[-1] == pytest.approx(1.2 * math.sqrt(3.) * 60. * KPC,
                                  rel=1e-15)
    assert y[-1] == 1. and y[0] == 0. and np.all(np.diff(y) > 0.)


def test_zero_density_packets_do_not_scatter(model):
    """tau_max = 0: the forced interaction has weight 0 and tau 0, interact
    returns end() at once - only the direct light, which is 1/(4 pi)."""
    ref = _restatement(model)
    tr = ref.trace(42, 0, 200, 4)
    assert np.all(tr[:, 0] == 1.) and np.all(tr[:, 1] == 0.)
    rows = tr[:, 4:12]
    assert np.all(rows[:, 7] == 0.25 / np.pi)


def test_source_gives_up_after_a_million_attempts(model):
    """A box around the origin too small for the source (the bulge starts at
    0.2 kpc, the disc lands within 1 pc of the centre with probability
    ~1e-11): the rejection loop stops after 1e6 attempts, the packet has no
    position (NaN) and a whole run counts it as dropped."""
    d = dict(model)
    d["anchor"] = [-0.001 * KPC] * 3
    d["sides"] = [0.002 * KPC] * 3
    ref = _restatement(d)
    out = ref.emit(42, 0, 2)
    assert np.all(np.isnan(out))
    image, counters = ref.shoot(42, 0, 2)
    assert counters[3] == 2 and counters[0] == 0
    assert np.all(image == 0.)
