"""`cmi-gpu --emission` with an AbsorptionSpectra: block on
the snapshot of a short lexington run, as the driver test of
test_gpu_absorbing_cube_driver.py builds it: two sightlines, one of them
towards a target inside the box, the two files, and their contents against
the Python call of the same arguments on the same state, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_image_lib as L
from test_gpu_absorbing_cube_driver import IONS, NCELL
from test_gpu_physics import lexington_engine

pytestmark = pytest.mark.gpu


def run(tmp_path, *args):
    exe = os.path.join(L.ROOT, "cmacionize_amd", "cmi-gpu")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    return r


def test_driver_writes_the_spectra_of_a_snapshot(tmp_path):
    import hdf5_mini
    import oracle_lib as o
    from cmacionize_amd import engine as E
    bench = os.path.join(L.ROOT, "benchmarks")
    text = open(os.path.join(bench, "lexingtonHII40.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((NCELL,) * 3))
    text = text.replace("number of photons: 1e8", "number of photons: 30000")
    text = text.replace("number of iterations: 20", "number of iterations: 6")
    text = text.replace("NumberDensity: 0", "NumberDensity: 1")
    shutil.copy(os.path.join(bench, "lexingtonHII40.yml"), tmp_path)
    (tmp_path / "run.param").write_text(text)
    run(tmp_path, "--params", "run.param")
    snapshot = str(tmp_path / "lexingtonHII40_006.hdf5")

    observer = (-2.5e17, 3.e16, 1.5e16)      # outside the box of +-5 pc
    direction = (2., -0.25, 0.125)
    target = (2.e16, -4.e16, 1.e16)          # inside it
    v_obs = (1e3, -2e3, 500.)
    names = ["HI_1215", "OI_1302", "OII_834", "SII_1259"]
    nchan, vmin, vmax = 96, -60e3, 60e3
    os.mkdir(tmp_path / "out")
    (tmp_path / "abs.param").write_text(
        "AbsorptionSpectra:\n  observer position: [%r m, %r m, %r m]\n"
        "  observer velocity: [%r m s^-1, %r m s^-1, %r m s^-1]\n"
        "  number of sightlines: 2\n"
        "  sightline direction 0: [%r, %r, %r]\n"
        "  target position 1: [%r m, %r m, %r m]\n"
        "  lines: [%s]\n  velocity channels: %d\n"
        "  velocity minimum: -60. km s^-1\n  velocity maximum: 60. km s^-1\n"
        "  turbulent velocity dispersion: 3. km s^-1\n"
        "  velocity field type: RadialExpansion\n"
        "  expansion velocity: 15. km s^-1\n  expansion radius: 5. pc\n"
        "  filename prefix: star\n  output folder: %s\n"
        % (observer + v_obs + direction + target +
           (", ".join(names), nchan, tmp_path / "out")))
    run(tmp_path, "--emission", "--params", "abs.param", "--file", snapshot)
    assert sorted(os.listdir(tmp_path / "out")) == [
        "star_absorption_columns.txt", "star_absorption_tau.dat"]
    used = open(str(tmp_path / "abs.param.used-values")).read()
    assert "number of sightlines: 2" in used
    assert "value not used" not in used

    # the same state on an engine of our own, every cell where its
    # coordinates put it
    f = hdf5_mini.read(snapshot)
    unit_length = 0.01 * float(np.ravel(
        f["/Units"].attrs["Unit length in cgs (U_L)"])[0])
    mid = f["/PartType0/Coordinates"].data.reshape(-1, 3) * unit_length
    idx = np.floor(NCELL * mid / (10. * o.PC)).astype(np.int64)
    cell = (idx[:, 0] * NCELL + idx[:, 1]) * NCELL + idx[:, 2]

    def placed(values):
        out = np.empty_like(values)
        out[..., cell] = values
        return out

    eng = lexington_engine(NCELL)
    eng.upload_cells(
        placed(f["/PartType0/NumberDensity"].data / unit_length ** 3),
        placed(f["/PartType0/Temperature"].data * float(np.ravel(
            f["/Units"].attrs["Unit temperature in cgs (U_T)"])[0])),
        placed(np.array([f["/PartType0/NeutralFraction" + i].data
                         for i in IONS])))
    # the block's velocity field at the cell centres, as the driver forms it
    side = 10. * o.PC / NCELL
    centre = -5. * o.PC + (np.arange(NCELL) + 0.5) * side
    r = np.stack(np.meshgrid(centre, centre, centre, indexing="ij"))
    eng.set_cell_velocities(((15e3 / (5. * o.PC)) * r).reshape(3, -1))
    # the sightlines as the driver forms them
    rays = []
    for d, length in ((np.array(direction), np.inf),
                      (np.array(target) - np.array(observer), None)):
        norm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        rays.append((d / norm, norm if length is None else length))
    tau, N = eng.render_absorption_spectra(
        names, observer, [x[0] for x in rays], nchan, vmin, vmax,
        lengths=[x[1] for x in rays], sigma_turb=3e3,
        observer_velocity=v_obs)
    eng.close()
    got = np.fromfile(str(tmp_path / "out" / "star_absorption_tau.dat"))
    assert got.shape == (2 * len(names) * nchan,)
    assert np.array_equal(got.reshape(2, len(names), nchan), tau)
    # the neutral gas around the nebula saturates Lyman alpha on the way
    # through the box; the sightline that ends at the star inside sees less
    assert tau[0, 0].max() > 10. and (N[1] < N[0]).all() and (N[1] > 0.).all()
    rows = [x.split() for x in open(str(
        tmp_path / "out" / "star_absorption_columns.txt")).read().splitlines()]
    assert [(int(x[0]), x[1]) for x in rows] == [
        (k, n) for k in range(2) for n in names]
    assert np.array_equal([float(x[2]) for x in rows], N.ravel())
    dv = (vmax - vmin) / nchan
    lam = E.absorption_table_lines(names)[4]
    W = E.equivalent_width(tau, dv, lam[None, :])
    # (the driver sums the channels one after the other, numpy in pairs)
    assert np.allclose([float(x[3]) for x in rows], W.ravel(),
                       rtol=nchan * 2. ** -53, atol=0.)
