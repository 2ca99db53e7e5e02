"""Absorption spectra without a GPU: the AbsorptionSpectra:
block of `cmi-gpu --emission` (directions and targets, its errors, what
--dry-run --describe prints, the driver's line table against the package's),
the numpy helpers against closed forms, and the CPU restatement
(tests/support/absorption_reference.c) against the contract in numpy."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import absorption_lib as AB
import scattered_line_lib as SL
from cmacionize_amd import engine as E

AXIS = ("  velocity channels: 16\n  velocity minimum: -80. km s^-1\n"
        "  velocity maximum: 80. km s^-1\n")
BLOCK = ("AbsorptionSpectra:\n"
         "  observer position: [1.e16 m, 2.e16 m, -3.e16 m]\n"
         "  number of sightlines: 2\n"
         "  sightline direction 0: [3., 0., 4.]\n"
         "  target position 1: [1.e16 m, 5.e16 m, 1.e16 m]\n"
         "  lines: [HI_1215, OI_1302, SII_1259]\n" + AXIS)


def _emission(tmp_path, text, *flags):
    params = tmp_path / "lines.param"
    params.write_text(text)
    cmd = [SL.CMI_GPU, "--emission"] + list(flags) + [
        "--params", str(params), "--file", str(tmp_path / "nowhere.hdf5")]
    return subprocess.run(cmd, capture_output=True, text=True,
                          cwd=str(tmp_path))


def test_describe_lists_the_block(tmp_path):
    """--dry-run --describe prints the block as JSON and needs no snapshot:
    the direction normalised, the target as a direction and a length, the
    lines with their constants"""
    r = _emission(tmp_path, BLOCK + "  observer velocity: [1. km s^-1, 0. km "
                  "s^-1, -2. km s^-1]\n  turbulent velocity dispersion: 3. km "
                  "s^-1\n  filename prefix: star\n", "--dry-run", "--describe")
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)["AbsorptionSpectra"]
    assert d["observer position"] == [1e16, 2e16, -3e16]
    assert d["observer velocity"] == [1e3, 0., -2e3]
    one, two = d["sightlines"]
    assert one == {"direction": [3. / 5., 0., 4. / 5.], "length": None}
    L = math.sqrt((0. * 0. + 3e16 * 3e16) + 4e16 * 4e16)
    assert two == {"direction": [0. / L, 3e16 / L, 4e16 / L], "length": L}
    assert [x["name"] for x in d["lines"]] == ["HI_1215", "OI_1302",
                                               "SII_1259"]
    assert d["velocity channels"] == 16
    assert d["velocity minimum"] == -80e3 and d["velocity maximum"] == 80e3
    assert d["turbulent velocity dispersion"] == 3e3
    assert d["velocity field type"] == "Static"
    assert d["filename prefix"] == "star" and d["output folder"] == "."


def test_driver_table_is_the_packages(tmp_path):
    """the driver's line table and the package's ABSORPTION_LINES are one
    table: ion, weight, wavelength, S and g of every line, bit for bit"""
    names = list(E.ABSORPTION_LINES)
    assert len(names) == 14
    assert sorted(E.ABSORPTION_LINES[n][0] for n in names) == list(range(14))
    text = BLOCK.replace("[HI_1215, OI_1302, SII_1259]",
                         "[" + ", ".join(names) + "]")
    r = _emission(tmp_path, text, "--dry-run", "--describe")
    assert r.returncode == 0, r.stderr
    lines = json.loads(r.stdout)["AbsorptionSpectra"]["lines"]
    ion, w, S, g, lam = E.absorption_table_lines(names)
    for k, row in enumerate(lines):
        assert row == {"name": names[k], "ion": int(ion[k]), "weight": w[k],
                       "wavelength": lam[k], "S": S[k], "g": g[k]}, names[k]
    # H I carries the Lyman-alpha mode's literals
    assert E.ABSORPTION_LINES["HI_1215"][1] == E.LYA_LAMBDA0
    assert E.ABSORPTION_LINES["HI_1215"][3] == 6.265e8


@pytest.mark.parametrize("change, message", [
    (("  sightline direction 0: [3., 0., 4.]\n",
      "  sightline direction 0: [3., 0., 4.]\n"
      "  target position 0: [0. m, 0. m, 0. m]\n"),
     "are both given"),
    (("  target position 1: [1.e16 m, 5.e16 m, 1.e16 m]\n", ""),
     "one of AbsorptionSpectra:sightline direction 1 and "
     "AbsorptionSpectra:target position 1 is required"),
    (("  observer position: [1.e16 m, 2.e16 m, -3.e16 m]\n", ""),
     "AbsorptionSpectra:observer position is required"),
    (("  lines: [HI_1215, OI_1302, SII_1259]\n", ""),
     "AbsorptionSpectra:lines is required"),
    (("OI_1302", "OI_1303"),
     "Unknown AbsorptionSpectra:lines entry \"OI_1303\""),
    (("  velocity channels: 16\n", ""),
     "AbsorptionSpectra:velocity channels is required"),
    (("  velocity maximum: 80. km s^-1\n", ""),
     "AbsorptionSpectra:velocity maximum is required"),
    (("[3., 0., 4.]", "[0., 0., 0.]"), "must be a finite vector"),
    (("[1.e16 m, 5.e16 m, 1.e16 m]", "[1.e16 m, 2.e16 m, -3.e16 m]"),
     "away from the observer"),
    (("number of sightlines: 2", "number of sightlines: 0"),
     "number of sightlines must be between"),
])
def test_driver_refuses(tmp_path, change, message):
    assert change[0] in BLOCK
    r = _emission(tmp_path, BLOCK.replace(*change), "--dry-run")
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr


def test_block_is_read_before_the_snapshot(tmp_path):
    """a good block gets as far as the snapshot, needs no flagged emission
    line, and its keys are listed as used"""
    r = _emission(tmp_path, BLOCK)
    assert r.returncode != 0 and "Could not open" in r.stderr, r.stderr
    used = open(str(tmp_path / "lines.param.used-values")).read()
    for word in ("AbsorptionSpectra:", "number of sightlines: 2",
                 "lines: [HI_1215, OI_1302, SII_1259]",
                 "velocity channels: 16", "filename prefix: absorption",
                 "turbulent velocity dispersion: 0 m s^-1",
                 "velocity field type: Static"):
        assert word in used, (word, used)
    assert "value not used" not in used


# ----------------------------------------------------------------- helpers --

def test_line_constants():
    """S = e^2 f lambda / (4 eps0 m_e c) = pi e^2 f lambda / (4 pi eps0 m_e
    c), the classical pi r_e c f lambda: 2.654e-6 m^2 s^-1 f lambda"""
    S, g = E.absorption_line_constants(1215.67e-10, 0.4164, 6.265e8)
    r_e = 2.8179403262e-15
    assert abs(S / (np.pi * r_e * 299792458. * 0.4164 * 1215.67e-10) - 1.) \
        < 1e-9
    assert g == 6.265e8 * 1215.67e-10 / (4. * np.pi)
    assert abs(g - 6.0608) < 1e-3      # m s^-1: a = 4.7e-4 at b = 12.9 km/s


def test_helpers_against_closed_forms():
    """an optically thin line has W = S N lambda0 / c, and the apparent
    column density inverts it; a saturated box line has W = its width"""
    lam, f = 1302.168e-10, 0.048
    S, _ = E.absorption_line_constants(lam, f, 5.65e8)
    nchan, vmin, vmax = 400, -100e3, 100e3
    dv = (vmax - vmin) / nchan
    v = E.cube_channel_centres(nchan, vmin, vmax)
    b, N = 10e3, 1e13      # m^-2: tau_0 = 9.4e-6
    tau = N * S * np.exp(-(v / b) ** 2) / (np.sqrt(np.pi) * b)
    assert tau.max() < 1e-5
    W = E.equivalent_width(tau, dv, lam)
    # thin: 1 - exp(-tau) = tau (1 - tau / 2 + ..), and the channel sum of a
    # Gaussian ten channels wide is its integral to better than 1e-12
    assert abs(W / (S * N * lam / 299792458.) - 1.) < tau.max()
    assert abs(E.apparent_column_density(tau, dv, S) / N - 1.) < 1e-10
    both = np.array([tau, 2. * tau])
    assert E.equivalent_width(both, dv, lam).shape == (2,)
    assert np.allclose(E.apparent_column_density(both, dv, S), [N, 2. * N],
                       rtol=1e-10)
    assert np.array_equal(E.transmitted_flux(both), np.exp(-both))
    box = np.where(np.abs(v) < 20e3, 1e3, 0.)
    assert abs(E.equivalent_width(box, dv, lam) -
               40e3 * lam / 299792458.) < 1e-12 * lam


# ---------------------------------------------------------- the restatement --

def test_restatement_against_numpy():
    """the restatement's spectrum of an axis-parallel ray is the sum of the
    contract's per-crossing terms formed in numpy (math.erf is libm's: the
    same bits), its N the sum of n ds; a ray cut at L adds the part of the
    last cell only"""
    box = AB.BOX
    n, b, vel = AB.random_lines(box, 7)
    o, d, ln = AB.sightlines(box)
    nc, vmin, vmax = AB.axis_of(65)
    tau, N = AB.spectra(box, n, b, AB.LINE_S, AB.LINE_G, o, d, ln, nc, vmin,
                        vmax, velocity=vel)
    assert AB.longest_ray <= 40
    # ray 0: along +x through the cells (i, 4, 3), ds = 0.25 each
    cells = (np.arange(11) * 9 + 4) * 7 + 3
    for l in range(3):
        want, col = np.zeros(nc), 0.
        for c in cells:
            if n[l, c] == 0.:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                want = want + AB.crossing_tau(n[l, c], 0.25, AB.LINE_S[l],
                                              AB.LINE_G[l], b[l, c],
                                              vel[0, c], nc, vmin, vmax)
            col = col + n[l, c] * 0.25
        assert N[0, l] == col
        assert np.allclose(tau[0, l], want, rtol=1e-13, atol=0.)
    # ray 1: along -z from above, L = 0.5 + 2.3 cells: cells (5, 4, 6..4)
    cells = (5 * 9 + 4) * 7 + np.array([6, 5, 4])
    ds = [0.375, 0.375, ln[1] - ((0.5 + 0.375) + 0.375)]
    assert abs(ds[2] - 0.3 * 0.375) < 1e-15
    for l in range(3):
        col = 0.
        for c, s in zip(cells, ds):
            if n[l, c] != 0.:
                col = col + n[l, c] * s
        assert N[1, l] == col
    # the rays that contribute nothing
    assert (tau[[7, 8, 9]] == 0.).all() and (N[[7, 8, 9]] == 0.).all()
    row = AB.probe(box, n[2], b[2], AB.LINE_S[2], AB.LINE_G[2], o[1], d[1],
                   8, nc, vmin, vmax, channels=[32, 40], length=ln[1],
                   velocity=vel)
    t0, t1, steps, pc, pds, run, end = AB.split_probe(row, 8, 2)
    assert (t0, t1, steps) == (0.5, 0.5 + 2.625, 3)
    assert list(pc[:3]) == list(cells) and list(pds[:3]) == ds
    assert np.array_equal(end, tau[1, 2, [32, 40]])
    assert np.array_equal(run[:, 2], end)
