"""`cmi-gpu --emission` with `Lyman alpha radiation field: true` and `HI Lyman
alpha coupling: true` on the snapshot of a short lexington run
of a thin gas (3 cm^-3: the box is ionized throughout and its H I has a
line-centre depth of a few tens, so that the run needs no core skipping): the
two files have the documented shapes and units, the H I cube is the Python call
with the spin temperature the driver wrote, bit for bit, and that spin
temperature is the one the Python entry points give for the same packets."""
import os
import subprocess

import numpy as np
import pytest

import line_image_lib as L
from test_gpu_physics import lexington_engine
from test_gpu_absorbing_cube_driver import IONS

pytestmark = pytest.mark.gpu

NCELL = 10
# no packet comes near it; a snapshot that went wrong fails, it does not hang
CAP = 100000
T_GAMMA = 2.725


def run(tmp_path, *args):
    exe = os.path.join(L.ROOT, "cmacionize_amd", "cmi-gpu")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    return r


def test_driver_writes_the_field_and_the_coupled_hi_cube(tmp_path):
    import hdf5_mini
    import oracle_lib as o
    bench = os.path.join(L.ROOT, "benchmarks")
    text = open(os.path.join(bench, "lexingtonHII40.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((NCELL,) * 3))
    text = text.replace("number of photons: 1e8", "number of photons: 20000")
    text = text.replace("number of iterations: 20", "number of iterations: 5")
    text = text.replace("NumberDensity: 0", "NumberDensity: 1")
    blocks = open(os.path.join(bench, "lexingtonHII40.yml")).read()
    assert "number density: 100. cm^-3" in blocks
    (tmp_path / "lexingtonHII40.yml").write_text(
        blocks.replace("number density: 100. cm^-3",
                       "number density: 3. cm^-3"))
    (tmp_path / "run.param").write_text(text)
    run(tmp_path, "--params", "run.param")
    snapshot = str(tmp_path / "lexingtonHII40_005.hdf5")

    nx, ny, nchan, npackets, seed = 9, 8, 10, 1500, 9
    theta, phi = 1.05, 0.5
    anchor, sides = (-2.8e17, -2.75e17), (5.6e17, 5.5e17)
    os.mkdir(tmp_path / "out")
    images = (
        "EmissivityValues:\n  Halpha: true\n"
        "EmissionImages:\n  view theta: %r radians\n  view phi: %r radians\n"
        "  image width: %d\n  image height: %d\n"
        "  anchor x: %r m\n  anchor y: %r m\n  sides x: %r m\n"
        "  sides y: %r m\n  output folder: %s\n"
        "  velocity channels: %d\n"
        "  velocity minimum: -60. km s^-1\n"
        "  velocity maximum: 60. km s^-1\n"
        "  turbulent velocity dispersion: 2. km s^-1\n"
        "  number of packets: %d\n  random seed: %d\n"
        "  HI cube: true\n  HI background temperature: %r K\n"
        "  Lyman alpha: true\n"
        "  Lyman alpha maximum scatterings: %d\n"
        % ((theta, phi, nx, ny) + anchor + sides +
           (tmp_path / "out", nchan, npackets, seed, T_GAMMA, CAP)))
    (tmp_path / "coupled.param").write_text(
        images + "  HI Lyman alpha coupling: true\n")
    run(tmp_path, "--emission", "--params", "coupled.param", "--file",
        snapshot)
    out = tmp_path / "out"
    written = sorted(os.listdir(out))
    assert "line_image_LymanAlpha_field.dat" in written
    assert "line_image_HI_spin_temperature.dat" in written
    used = open(str(tmp_path / "coupled.param.used-values")).read()
    assert "HI Lyman alpha coupling: true" in used
    assert "value not used" not in used
    n = NCELL ** 3
    field = np.fromfile(str(out / "line_image_LymanAlpha_field.dat"))
    T_s = np.fromfile(str(out / "line_image_HI_spin_temperature.dat"))
    assert field.shape == (5 * n,) and T_s.shape == (n,)
    field = field.reshape(5, n)
    cube = np.fromfile(str(out / "line_image_HI_cube.dat"))
    cube = cube.reshape(nchan, nx, ny)

    # the same state on an engine of our own (test_gpu_absorbing_cube_
    # driver.py), and the calls the driver makes
    f = hdf5_mini.read(snapshot)
    unit_length = 0.01 * float(np.ravel(
        f["/Units"].attrs["Unit length in cgs (U_L)"])[0])
    mid = f["/PartType0/Coordinates"].data.reshape(-1, 3) * unit_length
    idx = np.floor(NCELL * mid / (10. * o.PC)).astype(np.int64)
    cell = (idx[:, 0] * NCELL + idx[:, 1]) * NCELL + idx[:, 2]
    assert sorted(cell) == list(range(n))

    def placed(values):
        placed_ = np.empty_like(values)
        placed_[..., cell] = values
        return placed_

    density = placed(f["/PartType0/NumberDensity"].data / unit_length ** 3)
    T = placed(f["/PartType0/Temperature"].data * float(np.ravel(
        f["/Units"].attrs["Unit temperature in cgs (U_T)"])[0]))
    x = placed(np.array([f["/PartType0/NeutralFraction" + i].data
                         for i in IONS]))
    eng = lexington_engine(NCELL)
    eng.upload_cells(density, T, x)
    hi = dict(sigma_turb=2e3, background_temperature=T_GAMMA)
    args = (theta, phi, nx, ny, anchor, sides, nchan, -60e3, 60e3)
    assert np.array_equal(eng.render_hi_cube(*args, spin_temperature=T_s,
                                             **hi), cube)
    kinetic = eng.render_hi_cube(*args, **hi)
    assert not np.array_equal(kinetic, cube)

    eng.set_dust_scattering_per_hydrogen(0.5, 0., 0., 0.)
    eng.set_ccd_image(theta, phi, nx, ny, anchor, sides)
    eng.set_cell_source_field(eng.lyman_alpha_emissivity())
    eng.set_lyman_alpha(nchan, -60e3, 60e3, 2e3, 0., CAP)
    eng.set_lya_field()
    eng.lya_shoot(seed, 0, npackets)
    P, T_own = eng.lya_spin_temperature(npackets, T_GAMMA)
    ours = eng.lya_radiation_field(npackets)
    c = eng.get_lya_counters()
    eng.close()
    print("scatterings per packet", c["nhydrogen"] / npackets)
    assert c["ncapped"] == 0 and c["nhydrogen"] > npackets
    # two runs of the same packets: the order of the atomics
    assert np.allclose(T_s, T_own, rtol=1e-9, atol=0.)
    assert np.allclose(field[0], ours["energy_density"], rtol=1e-9, atol=0.)
    assert np.allclose(field[1], ours["scattering_rate"], rtol=1e-9, atol=0.)
    scale = np.abs(ours["force"]).max()
    assert np.allclose(field[2:], ours["force"], rtol=0., atol=1e-9 * scale)
    # units: J m^-3 of a nebula's Lyman alpha, a rate per atom that couples
    # the spin temperature to the gas wherever there is gas
    gas = (density > 0.) & (T > 0.)
    assert gas.sum() > 0.8 * n and (~gas).any()
    assert np.all(field[0] >= 0.) and (field[0] > 0.).mean() > 0.9
    assert 1e-20 < field[0].max() < 1e-6
    assert (field[1][gas] > 0.).mean() > 0.9
    assert np.all(field[1][density == 0.] == 0.)
    assert np.allclose(T_s[~gas], T_GAMMA, rtol=1e-15, atol=0.)
    lo, hi_ = np.minimum(T, T_GAMMA), np.maximum(T, T_GAMMA)
    assert np.all(T_s[gas] >= lo[gas] * (1. - 1e-12))
    assert np.all(T_s[gas] <= hi_[gas] * (1. + 1e-12))
    # the pressure pushes outwards
    centres = (np.stack(np.meshgrid(*[np.arange(NCELL)] * 3, indexing="ij"),
                        axis=-1).reshape(-1, 3) + 0.5) / NCELL - 0.5
    assert (field[2:].T * centres).sum() > 0.

    # the field alone: the same run, the H I cube with its kinetic temperature
    os.mkdir(tmp_path / "alone")
    (tmp_path / "alone.param").write_text(
        images.replace(str(out), str(tmp_path / "alone")) +
        "  Lyman alpha radiation field: true\n")
    run(tmp_path, "--emission", "--params", "alone.param", "--file", snapshot)
    alone = sorted(os.listdir(tmp_path / "alone"))
    assert "line_image_LymanAlpha_field.dat" in alone
    assert "line_image_HI_spin_temperature.dat" not in alone
    assert np.array_equal(np.fromfile(str(
        tmp_path / "alone" / "line_image_HI_cube.dat")).reshape(cube.shape),
        kinetic)
    again = np.fromfile(str(tmp_path / "alone" /
                            "line_image_LymanAlpha_field.dat")).reshape(5, n)
    assert np.allclose(again[0], field[0], rtol=1e-9, atol=0.)
