"""`cmi-gpu --emission` with `Lyman alpha: true` on the 14^3
snapshot of test_gpu_scattered_cube_driver.py's driver test: the Lyman-alpha
image and cube are written per view, the cube sums to no more than the image,
and a run without the key - absent or false - writes what it wrote: the same
files, the same snapshot, the same used-values. The neutral shell of the
snapshot has a line-centre depth of 1e7 and more, so the run skips the core
out to x_crit = 30."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scattered_line_lib as S

pytestmark = pytest.mark.gpu

NCHAN = 24
CHANNELS = ("  velocity channels: %d\n  velocity minimum: -3000. km s^-1\n"
            "  velocity maximum: 3000. km s^-1\n"
            "  turbulent velocity dispersion: 3. km s^-1\n"
            "  velocity field type: SolidBodyRotation\n"
            "  angular velocity: 1.e-13 s^-1\n" % NCHAN)


def _run(tmp_path, args):
    r = subprocess.run([S.CMI_GPU] + args, capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    return r


def test_driver_writes_the_lyman_alpha_image_and_cube(tmp_path):
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

    nx, ny = 12, 10
    switches = "EmissivityValues:\n  Halpha: true\n"
    images = ("EmissionImages:\n  view theta: 1.05 radians\n"
              "  view phi: 0.5 radians\n  image width: %d\n"
              "  image height: %d\n  filename prefix: %%s\n"
              "  output folder: %s\n  number of views: 2\n"
              "  view theta 1: 0.3 radians\n  view phi 1: 2. radians\n"
              % (nx, ny, str(tmp_path)) + CHANNELS)
    extra = ("  number of packets: 1500\n  random seed: 9\n"
             "  Lyman alpha core skipping: 30.\n"
             "  Lyman alpha maximum scatterings: 10000000\n")
    runs = {"absent": "", "off": "  Lyman alpha: false\n",
            "on": "  Lyman alpha: true\n" + extra}
    for name, key in runs.items():
        copy = str(tmp_path / (name + ".hdf5"))
        shutil.copy(snapshot, copy)
        (tmp_path / (name + ".param")).write_text(switches + images % name +
                                                  key)
        _run(tmp_path, ["--emission", "--params", name + ".param", "--file",
                        copy])

    def files(name):
        return sorted(n[len(name):] for n in os.listdir(tmp_path)
                      if n.startswith(name + "_"))

    assert files("absent") == files("off")
    assert not [n for n in files("absent") if "LymanAlpha" in n]
    for n in files("absent"):
        a = np.fromfile(str(tmp_path / ("absent" + n)))
        b = np.fromfile(str(tmp_path / ("off" + n)))
        assert np.array_equal(a, b), n
    assert open(str(tmp_path / "absent.hdf5"), "rb").read() == \
        open(str(tmp_path / "off.hdf5"), "rb").read() == \
        open(str(tmp_path / "on.hdf5"), "rb").read()
    absent = open(str(tmp_path / "absent.param.used-values")).read()
    off = open(str(tmp_path / "off.param.used-values")).read()
    assert "Lyman alpha" not in absent
    assert off.count("Lyman alpha: value not used") == 1
    assert [l for l in off.split("\n") if "Lyman alpha" not in l] == \
        [l.replace("absent", "off") for l in absent.split("\n")]

    new = [n for n in files("on") if n not in files("absent")]
    assert sorted(new) == sorted(
        "_LymanAlpha_%s%s.dat" % (kind, view)
        for kind in ("image", "cube") for view in ("", "_view1"))
    for n in files("absent"):
        a = np.fromfile(str(tmp_path / ("absent" + n)))
        b = np.fromfile(str(tmp_path / ("on" + n)))
        assert np.array_equal(a, b), n
    for view in ("", "_view1"):
        image = np.fromfile(str(
            tmp_path / ("on_LymanAlpha_image%s.dat" % view))).reshape(nx, ny)
        path = tmp_path / ("on_LymanAlpha_cube%s.dat" % view)
        assert path.stat().st_size == 8 * NCHAN * nx * ny
        cube = np.fromfile(str(path)).reshape(NCHAN, nx, ny)
        assert image.max() > 0. and np.all(image >= 0.)
        assert np.all(cube.sum(axis=0) <= image * (1. + 1e-12))
        assert cube.sum() > 0.5 * image.sum()
        # scattered out of the core: the light is spread over the channels
        assert np.count_nonzero(cube.sum(axis=(1, 2))) >= 4
