"""`cmi-gpu --emission` with the continuum keys in the EmissionImages and
EmissionSkyMaps blocks on the snapshot of a short lexington
run, as the driver test of test_gpu_sky_image.py builds it: the files are
written under the names of the further views and observers, the frequencies
are the logarithmic ladder, and every image is the Python call of the same
arguments on the same state, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import continuum_lib as K
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


def test_driver_writes_the_continuum_of_a_snapshot(tmp_path):
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

    nx, ny, s = 31, 26, 2
    views = [(1.05, 0.5), (0., 0.)]
    anchor, sides = (-2.8e17, -2.75e17), (5.6e17, 5.5e17)
    nlon, nlat = 40, 22
    lon, lat = (-1., 2.), (-0.5, 1.)
    observers = [(5.e16, -3.e16, 2.e16), (-1.e17, 1.e16, -5.e16)]
    os.mkdir(tmp_path / "out")
    text = (
        "EmissivityValues:\n  Halpha: true\n"
        "EmissionImages:\n  view theta: %r radians\n  view phi: %r radians\n"
        "  image width: %d\n  image height: %d\n  supersampling: %d\n"
        "  anchor x: %r m\n  anchor y: %r m\n  sides x: %r m\n"
        "  sides y: %r m\n  number of views: 2\n"
        "  view theta 1: %r radians\n  view phi 1: %r radians\n"
        "  output folder: %s\n"
        "  continuum frequencies: 5\n"
        "  continuum frequency minimum: 100. MHz\n"
        "  continuum frequency maximum: 30. GHz\n"
        "  continuum background temperature: 2.725 K\n"
        % (views[0] + (nx, ny, s) + anchor + sides + views[1] +
           (tmp_path / "out",)) +
        "EmissionSkyMaps:\n  observer position: [%r m, %r m, %r m]\n"
        "  number of longitude pixels: %d\n"
        "  number of latitude pixels: %d\n"
        "  longitude range: [%r radians, %r radians]\n"
        "  latitude range: [%r radians, %r radians]\n"
        "  number of observers: 2\n"
        "  observer position 1: [%r m, %r m, %r m]\n"
        "  output folder: %s\n"
        "  continuum frequencies: 1\n"
        "  continuum frequency minimum: 6. cm\n"
        "  continuum frequency maximum: 6. cm\n"
        % (observers[0] + (nlon, nlat) + lon + lat + observers[1] +
           (tmp_path / "out",)))
    (tmp_path / "continuum.param").write_text(text)
    run(tmp_path, "--emission", "--params", "continuum.param", "--file",
        snapshot)
    written = sorted(os.listdir(tmp_path / "out"))
    new = ["line_image_continuum.dat", "line_image_continuum_view1.dat",
           "line_image_continuum_frequencies.txt", "sky_map_continuum.dat",
           "sky_map_continuum_view1.dat",
           "sky_map_continuum_frequencies.txt"]
    lines = ["line_image_Halpha.dat", "line_image_Halpha_view1.dat",
             "sky_map_Halpha.dat", "sky_map_Halpha_view1.dat"]
    assert written == sorted(new + lines)
    used = open(str(tmp_path / "continuum.param.used-values")).read()
    assert "continuum frequencies: 5" in used
    assert "continuum frequency maximum: 3e+10 Hz # (30. GHz)" in used
    assert "value not used" not in used

    table = np.loadtxt(str(tmp_path / "out" /
                           "line_image_continuum_frequencies.txt"), ndmin=2)
    freq, bg = table[:, 0].copy(), table[:, 1].copy()
    want = K.driver_frequencies(5, 1e8, 3e10)
    assert freq[0] == 1e8 and np.allclose(freq, want, rtol=8 * K.EPS)
    assert np.allclose(bg, E.planck_function(freq, 2.725), rtol=16 * K.EPS)
    sky_table = np.loadtxt(str(tmp_path / "out" /
                               "sky_map_continuum_frequencies.txt"), ndmin=2)
    assert sky_table.shape == (1, 2) and sky_table[0, 1] == 0.
    assert abs(sky_table[0, 0] / (K.LIGHTSPEED / 0.06) - 1.) < 8 * K.EPS

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
    for k, (theta, phi) in enumerate(views):
        got = np.fromfile(str(tmp_path / "out" / (
            "line_image_continuum%s.dat" % ("_view1" if k else ""))))
        assert got.shape == (5 * nx * ny,)
        img = eng.render_continuum_images(freq, theta, phi, nx, ny, anchor,
                                          sides, s, background=bg)
        assert np.array_equal(got.reshape(5, nx, ny), img), k
        # the nebula stands out against the background: thick and at T_e at
        # 100 MHz, thin but there at 30 GHz
        assert (img.max(axis=(1, 2)) > bg).all()
        assert img[0].max() > 100. * bg[0]
        assert (img.min(axis=(1, 2)) == bg).all()
    for k, origin in enumerate(observers):
        got = np.fromfile(str(tmp_path / "out" / (
            "sky_map_continuum%s.dat" % ("_view1" if k else ""))))
        assert got.shape == (nlon * nlat,)
        sky = eng.render_continuum_sky_map(sky_table[:, 0], origin, nlon,
                                           nlat, lon, lat)
        assert sky.max() > 0.
        assert np.array_equal(got.reshape(1, nlon, nlat), sky), k
    eng.close()
