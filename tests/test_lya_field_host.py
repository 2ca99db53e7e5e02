"""The CPU restatement of the Lyman-alpha radiation field
(tests/support/lya_field_reference.c) and the host logic around it - no GPU.
The restatement is held to what follows from the contract (include/cmi_gpu.h,
"Lyman alpha radiation field"): the estimator identities, the
exact cases and the coupling formula; the driver to its keys, its refusals and
its unchanged used-values; the ABI to its three new entry points. The GPU
tests (test_gpu_lya_field.py) then hold the device to the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lya_field_lib as F
import lyman_alpha_lib as Y
import test_lyman_alpha_host as H

# the estimator identities: 16 batches of 250 packets of the stream SEED (the
# device's test, test_gpu_lya_field.py, runs the same)
SEED = 12
BATCHES = 16
BATCH = 250
SIGMAS = 4.


def identity_batches(shoot):
    """rows and momentum sums of the BATCHES batches; `shoot(first, n)`
    returns (rows [ncell][8], momentum [3] or None)"""
    out = [shoot(b * BATCH, BATCH) for b in range(BATCHES)]
    rows = np.array([r.sum(axis=0) for r, _ in out])  # [batch][8]
    momentum = None if out[0][1] is None else np.array([m for _, m in out])
    return rows, momentum


@pytest.mark.parametrize("x_crit", [0., 3.])
@pytest.mark.parametrize("dust", [True, False])
def test_estimator_identities(dust, x_crit):
    """sum_c S_H against sum_c N_H, the same for the dust, and without dust
    the momentum sum_c G_c against sum_packets forced (k_first - k_last): the
    track-length and the collision estimator of one quantity, and the two ways
    of counting the momentum a packet leaves behind (every hydrogen event
    takes the incoming k and re-emits isotropically). Each difference of the
    batch sums within SIGMAS standard errors of its batch mean of 0."""
    scene, _ = Y.parity_scene(dust=dust, x_crit=x_crit)
    ref = F.FieldRestatement(scene)

    def shoot(first, n):
        run = ref.shoot(SEED, first, n)
        assert run.counters["ncapped"] == 0
        return run.rows, run.momentum

    rows, momentum = identity_batches(shoot)
    assert rows[:, F.S_H].min() > 10. * BATCH / (1. + 20. * (x_crit > 0.))
    z_H = F.identity_sigmas(rows[:, F.S_H], rows[:, F.N_H])
    print("dust", dust, "x_crit", x_crit, "S_H - N_H:", z_H, "sigma; sums",
          rows[:, F.S_H].sum(), rows[:, F.N_H].sum())
    assert z_H <= SIGMAS
    if dust:
        assert rows[:, F.N_D].sum() > 100.
        z_d = F.identity_sigmas(rows[:, F.S_D], rows[:, F.N_D])
        print("S_d - N_d:", z_d, "sigma; sums", rows[:, F.S_D].sum(),
              rows[:, F.N_D].sum())
        assert z_d <= SIGMAS
    else:
        assert np.all(rows[:, F.S_D] == 0.) and np.all(rows[:, F.N_D] == 0.)
        z_G = F.identity_sigmas(rows[:, F.G_X:F.G_X + 3], momentum)
        print("G - forced (k_first - k_last):", z_G, "sigma; sums",
              rows[:, F.G_X:F.G_X + 3].sum(axis=0), momentum.sum(axis=0))
        assert np.all(z_G <= SIGMAS)


# -------------------------------------------------------- exact cases --

def transparent_scene(ncell=(6, 5, 7)):
    scene, _ = Y.parity_scene(ncell=ncell, nx=7, ny=5, dust=False)
    scene.n_HI[:] = 0.
    return scene


@pytest.mark.parametrize("ncell", [(6, 5, 7), (1, 1, 1)])
def test_a_transparent_box_tallies_the_chords(ncell):
    """kappa = 0 everywhere: l = ds exactly, so L sums to the packets' chord
    lengths; S, G and N are exactly 0, and nothing is NaN"""
    scene = transparent_scene(ncell)
    run = F.FieldRestatement(scene).shoot(SEED, 0, 2000)
    assert np.all(np.isfinite(run.rows))
    assert run.counters["nhydrogen"] == 0 and run.counters["ndust"] == 0
    assert run.chord > 0.
    assert abs(run.rows[:, F.L_].sum() / run.chord - 1.) <= 1e-12
    assert np.all(run.rows[:, 1:] == 0.)
    assert run.rows.shape == (int(np.prod(ncell)), 8)


def test_one_cell_with_hydrogen():
    """a 1 x 1 x 1 grid: every crossing is of the one cell; the identity holds
    there as well (to 4 standard errors of the packets)"""
    scene, _ = Y.parity_scene(ncell=(1, 1, 1), tau0=5., dust=False)
    ref = F.FieldRestatement(scene)
    rows = np.array([ref.shoot(SEED, k * 100, 100).rows[0]
                     for k in range(BATCHES)])
    assert np.all(np.isfinite(rows)) and rows[:, F.N_H].min() > 0.
    assert F.identity_sigmas(rows[:, F.S_H], rows[:, F.N_H]) <= SIGMAS


def test_dust_without_hydrogen_has_no_scattering_rate():
    """cells with n_HI = 0 but dust: S_d and N_d grow, S_H stays 0, and
    P_alpha is 0 there - not 0 / 0"""
    scene, _ = Y.parity_scene(ncell=(6, 5, 7), nx=7, ny=5, dust_tau=3.)
    scene.n_HI.reshape(-1)[::2] = 0.
    ref = F.FieldRestatement(scene)
    run = ref.shoot(SEED, 0, 2000)
    bare = scene.n_HI.reshape(-1) == 0.
    assert run.rows[bare, F.S_D].min() > 0. and run.rows[:, F.N_D].sum() > 0.
    assert np.all(run.rows[bare, F.S_H] == 0.)
    assert np.all(run.rows[bare, F.N_H] == 0.)
    P = ref.scattering_rate(run.rows, 1.0e20)
    assert np.all(P[bare] == 0.) and np.all(P[~bare] > 0.)
    assert np.all(np.isfinite(P))


# ------------------------------------------------------------ coupling --

T_GAMMA = 2.725
LATTICE_T = [0.5, 1., 10., 32., 150., 2.0e3, 1.0e4, 3.0e4, 1.0e6]
LATTICE_N_HI = [0., 1., 1.0e6, 1.0e12]
LATTICE_N_E = [0., 1.0e2, 1.0e8]
LATTICE_P = [0., 1.0e-14, 1.0e-13, 1.0e-12, 1.0e-11, 1.0e-8, 1., 1.0e30]


def lattice():
    T, n_HI, n_e, P = (a.reshape(-1) for a in np.meshgrid(
        LATTICE_T, LATTICE_N_HI, LATTICE_N_E, LATTICE_P, indexing="ij"))
    return T, n_HI, n_e, P


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("collisions", [True, False])
def test_coupling_formula_against_numpy(collisions):
    T, n_HI, n_e, P = lattice()
    got = F.spin_temperature_c(T, n_HI, n_e, P, T_GAMMA, collisions)
    expect = F.spin_temperature_numpy(T, n_HI, n_e, P, T_GAMMA, collisions)
    worst = ulps(got, expect)
    print("collisions", collisions, "worst", worst.max(), "ulp at",
          [v[np.argmax(worst)] for v in (T, n_HI, n_e, P)])
    assert np.all(np.isfinite(got))
    assert worst.max() <= 4.
    # T_s lies between the background and the kinetic temperature
    lo, hi = np.minimum(T, T_GAMMA), np.maximum(T, T_GAMMA)
    assert np.all(got >= lo * (1. - 4. * np.finfo(float).eps))
    assert np.all(got <= hi * (1. + 4. * np.finfo(float).eps))
    # and the lattice has every regime: uncoupled, partly, fully coupled
    x = F.coupling(T, n_HI, n_e, T_GAMMA, collisions, P)
    assert (x < 1e-3).any() and ((x > 0.1) & (x < 10.)).any() and \
        (x > 1e6).any()


def test_coupling_limits():
    T = np.array(LATTICE_T)
    zero = np.zeros(len(T))
    # no Lyman alpha, no collisions: the background
    got = F.spin_temperature_c(T, 1.0e6, 1.0e2, zero, T_GAMMA, False)
    assert np.array_equal(got, np.full(len(T), T_GAMMA))
    # P_alpha -> infinity: the kinetic temperature
    got = F.spin_temperature_c(T, 1.0e6, 1.0e2, zero + 1.0e30, T_GAMMA, True)
    assert ulps(got, T).max() <= 4.
    # a cell without a temperature gets the background
    got = F.spin_temperature_c(np.array([0., -5.]), 1.0e6, 1.0e2, 1.0e-9,
                               T_GAMMA, True)
    assert np.array_equal(got, [T_GAMMA, T_GAMMA])
    # the rate coefficients at the values their papers quote: kappa_HH(100 K)
    # = 3.1e-11 100^0.357 exp(-0.32) = 1.17e-10 cm^3 s^-1; Liszt's kappa_eH
    # is 10^-9.607 at 1 K and flat above 1e4 K
    assert abs(F.kappa_HH(100.) / 1.166e-16 - 1.) < 2e-3
    assert abs(F.kappa_eH(1.) / 10. ** -15.607 - 1.) < 1e-12
    assert F.kappa_eH(5.0e4) == F.kappa_eH(1.0e4) and \
        F.kappa_eH(0.1) == F.kappa_eH(1.)


# -------------------------------------------------------------- driver --

LYA = H.CHANNELS + H.KEY % "true"
HI = "  HI cube: true\n"
FIELD = "  Lyman alpha radiation field: %s\n"
COUPLING = "  HI Lyman alpha coupling: %s\n"
BACKGROUND = "  HI background temperature: 2.725 K\n"


@pytest.mark.parametrize("text, words", [
    (H.IMAGES + LYA + HI + BACKGROUND + COUPLING % "true" +
     "  Lyman alpha core skipping: 3.\n" + H.SKY,
     ("EmissionImages:HI Lyman alpha coupling",
      "EmissionImages:Lyman alpha core skipping")),
    (H.IMAGES + LYA + HI + BACKGROUND + COUPLING % "true" +
     "  HI spin temperature type: Fixed\n  HI spin temperature: 100. K\n" +
     H.SKY,
     ("EmissionImages:HI Lyman alpha coupling",
      "EmissionImages:HI spin temperature type", "Fixed")),
    (H.IMAGES + LYA + HI + COUPLING % "true" + H.SKY,
     ("EmissionImages:HI Lyman alpha coupling",
      "EmissionImages:HI background temperature")),
    (H.IMAGES + LYA + HI + "  HI background temperature: 0. K\n" +
     COUPLING % "true" + H.SKY,
     ("EmissionImages:HI Lyman alpha coupling",
      "EmissionImages:HI background temperature")),
])
def test_driver_refuses(tmp_path, text, words):
    r, used = H._emission(tmp_path, text)
    assert r.returncode != 0, r.stderr
    for word in words:
        assert word in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(used)


def _used(tmp_path, text):
    r, used = H._emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    return open(used).read()


def test_driver_lists_the_keys_only_with_their_switches(tmp_path):
    both = _used(tmp_path, H.IMAGES + LYA + HI + BACKGROUND + FIELD % "true" +
                 COUPLING % "true" + H.SKY)
    assert both.count("Lyman alpha radiation field: true") == 1
    assert both.count("HI Lyman alpha coupling: true") == 1
    # the Lyman-alpha run without the new keys: they are not listed
    plain = _used(tmp_path, H.IMAGES + LYA + HI + BACKGROUND + H.SKY)
    assert "radiation field" not in plain and "coupling" not in plain
    # the keys without "Lyman alpha: true" are not read
    off = _used(tmp_path, H.IMAGES + H.CHANNELS + HI + BACKGROUND +
                FIELD % "true" + COUPLING % "true" + H.SKY)
    assert off.count("Lyman alpha radiation field: value not used") == 1
    assert off.count("HI Lyman alpha coupling: value not used") == 1
    # the coupling without the H I cube is not read either
    lonely = _used(tmp_path, H.IMAGES + LYA + COUPLING % "true" + H.SKY)
    assert lonely.count("HI Lyman alpha coupling: value not used") == 1
    # a key that is false is listed as read, and changes nothing else
    false = _used(tmp_path, H.IMAGES + LYA + HI + BACKGROUND +
                  FIELD % "false" + COUPLING % "false" + H.SKY)
    assert [l for l in false.split("\n")
            if "radiation field" not in l and "coupling" not in l] == \
        plain.split("\n")
    # the sky maps' H I cube is not coupled: the key is not read there
    sky = _used(tmp_path, H.IMAGES + LYA + H.SKY + H.CHANNELS + HI +
                COUPLING % "true")
    assert sky.count("HI Lyman alpha coupling: value not used") == 1


def test_golden_used_values_are_unchanged(tmp_path):
    """a file that sets none of the new keys: byte for byte what it was"""
    assert _used(tmp_path, H.ONE_VIEW) == \
        open(os.path.join(H.GOLDEN, "one_view_lines.param.usedvalues")).read()


# ----------------------------------------------------------------- ABI --

NEW_SYMBOLS = ("cmi_gpu_set_lya_field", "cmi_gpu_download_lya_field",
               "cmi_gpu_lya_spin_temperature")


def test_the_new_entry_points_are_in_header_binding_and_library():
    from cmacionize_amd import engine
    text = open(os.path.join(os.path.dirname(H.SL.HERE), "include",
                             "cmi_gpu.h")).read()
    code = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    code = re.sub(r"\s+([,)])", r"\1", code)
    lib = C.CDLL(engine.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(cmi_gpu_engine \*engine" % name, code)
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert ("int cmi_gpu_lya_spin_temperature(cmi_gpu_engine *engine, double "
            "luminosity_per_packet, double background_temperature, int32_t "
            "collisions, double *P_alpha, double *T_s);") in code
    # the entry point the field leans on keeps its signature
    assert ("int cmi_gpu_get_lya_counters(cmi_gpu_engine *engine, uint64_t "
            "*counters);") in code
