"""`cmi-gpu --emission` with the spectral-cube keys of the EmissionSkyMaps
block on the snapshot of a short lexington run, as the
driver test of test_gpu_line_cube_driver.py builds it: the cube files have the
right size and sum to the integrated maps, a second observer with another
velocity sees the dipole of the difference, and a file without the new keys
gives what it gave."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_image_lib as L

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NCELL = 14


def run(tmp_path, *args, fails=False):
    exe = os.path.join(L.ROOT, "cmacionize_amd", "cmi-gpu")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert (r.returncode != 0) == fails, r.stderr
    return r


def test_driver_writes_the_sky_cubes_of_a_snapshot(tmp_path):
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

    nlon, nlat, nchan = 24, 12, 120
    os.mkdir(tmp_path / "with")
    os.mkdir(tmp_path / "without")
    switches = ("EmissivityValues:\n  Halpha: true\n  OIII_5007: true\n"
                "  WFC2_F555W: true\n")
    position = "[1. pc, -0.5 pc, 0.3 pc]"
    block = ("EmissionSkyMaps:\n  observer position: %s\n"
             "  number of longitude pixels: %d\n"
             "  number of latitude pixels: %d\n"
             "  dust cross section per hydrogen: 2.e-27 m^2\n"
             "  number of observers: 2\n  observer position 1: %s\n"
             "  output folder: %%s\n" % (position, nlon, nlat, position))
    dv_obs = np.array([30.e3, -20.e3, 10.e3])
    cube_keys = ("  velocity channels: %d\n"
                 "  velocity minimum: -300. km s^-1\n"
                 "  velocity maximum: 300. km s^-1\n"
                 "  velocity field type: RadialExpansion\n"
                 "  expansion velocity: 20. km s^-1\n"
                 "  expansion radius: 5. pc\n"
                 "  expansion centre: %s\n"
                 "  observer velocity: [1. km s^-1, 2. km s^-1, -3. km s^-1]\n"
                 "  observer velocity 1: [31. km s^-1, -18. km s^-1, "
                 "7. km s^-1]\n" % (nchan, position))
    (tmp_path / "cubes.param").write_text(
        switches + block % (tmp_path / "with") + cube_keys)
    (tmp_path / "maps.param").write_text(
        switches + block % (tmp_path / "without"))
    r = run(tmp_path, "--emission", "--params", "cubes.param", "--file",
            snapshot)
    assert "WFC2_F555W is not the line of one ion" in r.stderr
    run(tmp_path, "--emission", "--params", "maps.param", "--file", snapshot)

    with_keys = sorted(os.listdir(tmp_path / "with"))
    without = sorted(os.listdir(tmp_path / "without"))
    names = ["sky_map_%s%s.dat" % (line, view)
             for line in ("Halpha", "OIII_5007", "WFC2_F555W")
             for view in ("", "_view1")]
    cubes = ["sky_map_%s_cube%s.dat" % (line, view)
             for line in ("Halpha", "OIII_5007") for view in ("", "_view1")]
    assert without == sorted(names)
    assert with_keys == sorted(names + cubes)
    # the keys change none of the other outputs
    for name in names:
        assert open(str(tmp_path / "with" / name), "rb").read() == \
            open(str(tmp_path / "without" / name), "rb").read(), name
    used = open(str(tmp_path / "maps.param.used-values")).read()
    assert "velocity" not in used and "expansion" not in used
    used = open(str(tmp_path / "cubes.param.used-values")).read()
    assert "velocity channels: %d" % nchan in used
    assert "observer velocity 1: [31000 m s^-1, -18000 m s^-1, 7000 m s^-1]" \
        in used

    # +-300 km/s covers u +- 6 b of every cell (|u| < 90 km/s with the
    # observers' velocities, b < 20 km/s up to 24000 K for hydrogen): the
    # channels sum to the map as in case 5 of test_gpu_sky_cube.py; a ray
    # crosses at most 3 NCELL cells
    allowed = (nchan + 8 * 3 * NCELL) * EPS
    centres = E.cube_channel_centres(nchan, -300.e3, 300.e3)
    d, _ = E.sky_map_directions(nlon, nlat)
    dipole = (d @ dv_obs).reshape(nlon, nlat)
    for line in ("Halpha", "OIII_5007"):
        mean = {}
        for view in ("", "_view1"):
            cube = np.fromfile(str(tmp_path / "with" / (
                "sky_map_%s_cube%s.dat" % (line, view))))
            assert cube.shape == (nchan * nlon * nlat,)
            cube = cube.reshape(nchan, nlon, nlat)
            sky = np.fromfile(str(tmp_path / "with" / (
                "sky_map_%s%s.dat" % (line, view)))).reshape(nlon, nlat)
            assert (sky > 0.).all()   # the observer is inside
            err = (np.abs(cube.sum(axis=0) - sky) / sky).max()
            print(line, view, "worst", err, "allowed", allowed)
            assert err <= allowed
            assert (cube.sum(axis=(1, 2)) > 0.).sum() >= 2
            assert not cube[0].any() and not cube[-1].any()
            _, mean[view], _ = E.cube_moments(cube, centres)
        # the same place, another velocity: u_1 = u_0 - (v_1 - v_0) . d
        shift = mean["_view1"] - (mean[""] - dipole)
        print(line, "worst shift off the dipole", np.abs(shift).max(),
              "channel width", centres[1] - centres[0])
        assert (np.abs(shift) <= centres[1] - centres[0]).all()
        assert np.abs(dipole).max() > 5. * (centres[1] - centres[0])
        # the expansion is about the observer: everything recedes
        assert (mean[""] > 0.).mean() > 0.9
