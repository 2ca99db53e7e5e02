"""`cmi-gpu --emission` with `scattered cubes: true` on the
14^3 snapshot of test_gpu_scattered_line.py's driver test: the cubes of the
scattered light are written for both blocks, they sum to the scattered
images, and a run without the key - absent or false - writes what it wrote:
the same files, the same snapshot, the same used-values."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scattered_line_lib as S

pytestmark = pytest.mark.gpu

NCHAN = 5
CHANNELS = ("  velocity channels: %d\n  velocity minimum: -200. km s^-1\n"
            "  velocity maximum: 200. km s^-1\n"
            "  turbulent velocity dispersion: 3. km s^-1\n"
            "  velocity field type: SolidBodyRotation\n"
            "  angular velocity: 1.e-13 s^-1\n" % NCHAN)


def _run(tmp_path, args):
    r = subprocess.run([S.CMI_GPU] + args, capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    return r


def test_driver_writes_the_scattered_cubes(tmp_path):
    bench = os.path.join(S.ROOT, "benchmarks")
    ncell = 14
    text = open(os.path.join(bench, "lexingtonHII40.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((ncell,) * 3))
    text = text.replace("number of photons: 1e8", "number of photons: 30000")
    text = text.replace("number of iterations: 20", "number of iterations: 6")
    text = text.replace("NumberDensity: 0", "NumberDensity: 1")
    shutil.copy(os.path.join(bench, "lexingtonHII40.yml"), tmp_path)
    (tmp_path / "run.param").write_text(text)
    _run(tmp_path, ["--params", "run.param"])
    snapshot = str(tmp_path / "lexingtonHII40_006.hdf5")

    nx, ny, nlon, nlat = 24, 20, 16, 8
    switches = "EmissivityValues:\n  Halpha: true\n  HII: true\n"
    scattering = ("  dust cross section per hydrogen: 2.e-27 m^2\n"
                  "  scattering: true\n  number of packets: 20000\n"
                  "  random seed: 9\n  dust albedo: 0.54\n"
                  "  dust asymmetry: 0.44\n"
                  "  dust peak linear polarisation: 0.43\n")
    images = ("EmissionImages:\n  view theta: 1.05 radians\n"
              "  view phi: 0.5 radians\n  image width: %d\n"
              "  image height: %d\n  filename prefix: %%s\n"
              "  output folder: %s\n" % (nx, ny, str(tmp_path)) + scattering +
              CHANNELS)
    sky = ("EmissionSkyMaps:\n  observer position: [1.e16 m, 2.e16 m, -3.e16 m]"
           "\n  observer velocity: [2. km s^-1, 0. km s^-1, -1. km s^-1]\n"
           "  number of longitude pixels: %d\n"
           "  number of latitude pixels: %d\n  exclusion radius: 1.e16 m\n"
           "  filename prefix: %%ssky\n  output folder: %s\n" %
           (nlon, nlat, str(tmp_path)) + scattering + CHANNELS)
    runs = {"absent": "", "off": "  scattered cubes: false\n",
            "on": "  scattered cubes: true\n"}
    for name, key in runs.items():
        copy = str(tmp_path / (name + ".hdf5"))
        shutil.copy(snapshot, copy)
        (tmp_path / (name + ".param")).write_text(
            switches + images % name + key + sky % name + key)
        _run(tmp_path, ["--emission", "--params", name + ".param", "--file",
                        copy])

    def files(name):
        return sorted(n[len(name):] for n in os.listdir(tmp_path)
                      if n.startswith(name + "_") or
                      n.startswith(name + "sky_"))

    # without the key, absent or false: the same files with the same bytes
    # where no atomic is involved, the same snapshot, the same used-values
    # but for the line that says the key was not used
    assert files("absent") == files("off")
    assert not [n for n in files("absent") if "scattered_cube" in n]
    for n in files("absent"):
        a = np.fromfile(str(tmp_path / ("absent" + n)))
        b = np.fromfile(str(tmp_path / ("off" + n)))
        if "scattered" in n:
            assert np.allclose(a, b, rtol=1e-12,
                               atol=1e-14 * np.abs(a).max()), n
        else:
            assert np.array_equal(a, b), n
    assert open(str(tmp_path / "absent.hdf5"), "rb").read() == \
        open(str(tmp_path / "off.hdf5"), "rb").read() == \
        open(str(tmp_path / "on.hdf5"), "rb").read()
    absent = open(str(tmp_path / "absent.param.used-values")).read()
    off = open(str(tmp_path / "off.param.used-values")).read()
    assert "scattered cubes" not in absent
    assert off.count("scattered cubes: value not used") == 2
    assert [l for l in off.split("\n") if "scattered cubes" not in l] == \
        [l.replace("absent", "off") for l in absent.split("\n")]

    # with it: six more files (HII is not the line of one ion: no cube), the
    # others as they were
    new = [n for n in files("on") if n not in files("absent")]
    assert sorted(new) == sorted(
        "%s_Halpha_scattered_cube_%s.dat" % (block, stokes)
        for block in ("", "sky") for stokes in "IQU")
    for n in files("absent"):
        a = np.fromfile(str(tmp_path / ("absent" + n)))
        b = np.fromfile(str(tmp_path / ("on" + n)))
        assert np.allclose(a, b, rtol=1e-12, atol=1e-14 * np.abs(a).max()), n
    # the axis covers the line: the cubes sum to the scattered images
    for block, shape in (("", (nx, ny)), ("sky", (nlon, nlat))):
        top = np.abs(np.fromfile(str(
            tmp_path / ("on%s_Halpha_scattered_I.dat" % block)))).max()
        assert top > 0.
        for stokes in "IQU":
            path = tmp_path / ("on%s_Halpha_scattered_cube_%s.dat" %
                               (block, stokes))
            assert path.stat().st_size == 8 * NCHAN * shape[0] * shape[1]
            cube = np.fromfile(str(path)).reshape((NCHAN,) + shape)
            image = np.fromfile(str(
                tmp_path / ("on%s_Halpha_scattered_%s.dat" % (block, stokes))
            )).reshape(shape)
            assert np.allclose(cube.sum(axis=0), image, rtol=1e-12,
                               atol=1e-14 * top), (block, stokes)
            if stokes == "I":
                # and the light is spread over the channels, not in one
                assert np.count_nonzero(cube.sum(axis=(1, 2))) >= 3
