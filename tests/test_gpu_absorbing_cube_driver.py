"""`cmi-gpu --emission` with `HI cube: true` in the EmissionImages and
EmissionSkyMaps blocks on the snapshot of a short lexington
run, as the driver test of test_gpu_continuum_driver.py builds it: the files
are written under the names of the further views and observers, and every
cube is the Python call of the same arguments on the same state, bit for
bit; a velocity field of the block reaches the H I cube even when no line
has a cube of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_image_lib as L
from test_gpu_physics import lexington_engine

pytestmark = pytest.mark.gpu

NCELL = 14
IONS = ["H", "He", "C+", "C++", "N", "N+", "N++", "O", "O+", "Ne", "Ne+",
        "S+", "S++", "S+++"]


def run(tmp_path, *args):
    exe = os.path.join(L.ROOT, "cmacionize_amd", "cmi-gpu")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    return r


def test_driver_writes_the_hi_cubes_of_a_snapshot(tmp_path):
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

    nx, ny, s, nchan = 31, 26, 2, 12
    views = [(1.05, 0.5), (0., 0.)]
    anchor, sides = (-2.8e17, -2.75e17), (5.6e17, 5.5e17)
    nlon, nlat = 40, 22
    lon, lat = (-1., 2.), (-0.5, 1.)
    observers = [(5.e16, -3.e16, 2.e16), (-1.e17, 1.e16, -5.e16)]
    velocities = [(1e3, 2e3, -3e3), (31e3, -18e3, 7e3)]
    os.mkdir(tmp_path / "out")
    images = (
        "EmissivityValues:\n  WFC2_F555W: true\n"
        "EmissionImages:\n  view theta: %r radians\n  view phi: %r radians\n"
        "  image width: %d\n  image height: %d\n  supersampling: %d\n"
        "  anchor x: %r m\n  anchor y: %r m\n  sides x: %r m\n"
        "  sides y: %r m\n  number of views: 2\n"
        "  view theta 1: %r radians\n  view phi 1: %r radians\n"
        "  output folder: %s\n"
        "  velocity channels: %d\n"
        "  velocity minimum: -40. km s^-1\n"
        "  velocity maximum: 40. km s^-1\n"
        "  turbulent velocity dispersion: 2. km s^-1\n"
        "  HI cube: true\n"
        "  HI spin temperature type: Fixed\n"
        "  HI spin temperature: 100. K\n"
        "  HI background temperature: 2.725 K\n"
        % (views[0] + (nx, ny, s) + anchor + sides + views[1] +
           (tmp_path / "out", nchan)))
    text = images + (
        "EmissionSkyMaps:\n  observer position: [%r m, %r m, %r m]\n"
        "  number of longitude pixels: %d\n"
        "  number of latitude pixels: %d\n"
        "  longitude range: [%r radians, %r radians]\n"
        "  latitude range: [%r radians, %r radians]\n"
        "  number of observers: 2\n"
        "  observer position 1: [%r m, %r m, %r m]\n"
        "  output folder: %s\n"
        "  velocity channels: %d\n"
        "  velocity minimum: -60. km s^-1\n"
        "  velocity maximum: 60. km s^-1\n"
        "  observer velocity: [%r m s^-1, %r m s^-1, %r m s^-1]\n"
        "  observer velocity 1: [%r m s^-1, %r m s^-1, %r m s^-1]\n"
        "  HI cube: true\n"
        "  HI free-free continuum: false\n"
        % (observers[0] + (nlon, nlat) + lon + lat + observers[1] +
           (tmp_path / "out", nchan) + velocities[0] + velocities[1]))
    (tmp_path / "hi.param").write_text(text)
    r = run(tmp_path, "--emission", "--params", "hi.param", "--file",
            snapshot)
    assert "WFC2_F555W is not the line of one ion" in r.stderr
    written = sorted(os.listdir(tmp_path / "out"))
    new = ["line_image_HI_cube.dat", "line_image_HI_cube_view1.dat",
           "sky_map_HI_cube.dat", "sky_map_HI_cube_view1.dat"]
    lines = ["line_image_WFC2_F555W.dat", "line_image_WFC2_F555W_view1.dat",
             "sky_map_WFC2_F555W.dat", "sky_map_WFC2_F555W_view1.dat"]
    assert written == sorted(new + lines)
    used = open(str(tmp_path / "hi.param.used-values")).read()
    assert "HI cube: true" in used and "HI spin temperature: 100 K" in used
    assert "value not used" not in used

    # the same state on an engine of our own, every cell where its
    # coordinates put it
    f = hdf5_mini.read(snapshot)
    unit_length = 0.01 * float(np.ravel(
        f["/Units"].attrs["Unit length in cgs (U_L)"])[0])
    mid = f["/PartType0/Coordinates"].data.reshape(-1, 3) * unit_length
    idx = np.floor(NCELL * mid / (10. * o.PC)).astype(np.int64)
    cell = (idx[:, 0] * NCELL + idx[:, 1]) * NCELL + idx[:, 2]
    assert sorted(cell) == list(range(NCELL ** 3))

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
    static = {}
    for k, (theta, phi) in enumerate(views):
        got = np.fromfile(str(tmp_path / "out" / (
            "line_image_HI_cube%s.dat" % ("_view1" if k else ""))))
        assert got.shape == (nchan * nx * ny,)
        cube = eng.render_hi_cube(theta, phi, nx, ny, anchor, sides, nchan,
                                  -40e3, 40e3, s, sigma_turb=2e3,
                                  spin_temperature=100.,
                                  background_temperature=2.725)
        assert np.array_equal(got.reshape(nchan, nx, ny), cube), k
        static[k] = cube
        # the neutral gas around the nebula is there, at rest, in the middle
        # channels, in front of the background; the outer channels show the
        # background and the nebula's free-free continuum
        bg = E.planck_function(E.HI_FREQUENCY, 2.725)
        T_b = E.brightness_temperature(cube, E.HI_FREQUENCY)
        assert cube.min() >= 0.99 * bg
        assert (T_b[nchan // 2] - T_b[0]).max() > 3.
        assert T_b[0].max() > 3. * T_b[0].min()
    for k, origin in enumerate(observers):
        got = np.fromfile(str(tmp_path / "out" / (
            "sky_map_HI_cube%s.dat" % ("_view1" if k else ""))))
        assert got.shape == (nchan * nlon * nlat,)
        sky = eng.render_hi_sky_map_cube(origin, nlon, nlat, nchan, -60e3,
                                         60e3, lon, lat, free_free=False,
                                         observer_velocity=velocities[k])
        assert sky.max() > 0.
        assert np.array_equal(got.reshape(nchan, nlon, nlat), sky), k
    eng.close()

    # a velocity field of the block reaches the H I cube although no flagged
    # entry has a cube of its own: the expanding shell splits the line
    os.mkdir(tmp_path / "moving")
    text = images.replace(str(tmp_path / "out"), str(tmp_path / "moving")) + (
        "  velocity field type: RadialExpansion\n"
        "  expansion velocity: 20. km s^-1\n"
        "  expansion radius: 5. pc\n")
    (tmp_path / "moving.param").write_text(text)
    run(tmp_path, "--emission", "--params", "moving.param", "--file",
        snapshot)
    moving = np.fromfile(str(tmp_path / "moving" / "line_image_HI_cube.dat"))
    moving = moving.reshape(nchan, nx, ny)
    assert not np.array_equal(moving, static[0])
    centres = E.cube_channel_centres(nchan, -40e3, 40e3)
    # (the line alone: less the first channel, which holds the continuum)
    spread = [np.sqrt(((c - c[0]).clip(0.).sum(axis=(1, 2)) *
                       centres ** 2).sum() / (c - c[0]).clip(0.).sum())
              for c in (static[0], moving)]
    print("rms velocity of the line, at rest and expanding:", spread)
    assert spread[1] > 1.3 * spread[0]
