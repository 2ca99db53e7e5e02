"""`cmi-gpu --emission` with the spectral-cube keys of the EmissionImages
block on the snapshot of a short lexington run, as the
driver test of test_gpu_line_image.py builds it: the cube files have the
right size and sum to the integrated images, and a file without the new keys
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


def test_driver_writes_the_cubes_of_a_snapshot(tmp_path):
    import hdf5_mini
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
    plain = str(tmp_path / "plain.hdf5")
    shutil.copy(snapshot, plain)

    nx, ny, nchan = 31, 26, 8
    os.mkdir(tmp_path / "with")
    os.mkdir(tmp_path / "without")
    switches = ("EmissivityValues:\n  Halpha: true\n  OIII_5007: true\n"
                "  WFC2_F555W: true\n")
    block = ("EmissionImages:\n  view theta: 1.05 radians\n"
             "  view phi: 0.5 radians\n  image width: %d\n"
             "  image height: %d\n  supersampling: 2\n"
             "  dust cross section per hydrogen: 2.e-27 m^2\n"
             "  number of views: 2\n  view theta 1: 0. radians\n"
             "  view phi 1: 0. radians\n  output folder: %s\n")
    cube_keys = ("  velocity channels: %d\n"
                 "  velocity minimum: -300. km s^-1\n"
                 "  velocity maximum: 300. km s^-1\n"
                 "  velocity field type: RadialExpansion\n"
                 "  expansion velocity: 20. km s^-1\n"
                 "  expansion radius: 5. pc\n" % nchan)
    (tmp_path / "cubes.param").write_text(
        switches + block % (nx, ny, tmp_path / "with") + cube_keys)
    (tmp_path / "images.param").write_text(
        switches + block % (nx, ny, tmp_path / "without"))
    r = run(tmp_path, "--emission", "--params", "cubes.param", "--file",
            snapshot)
    assert "WFC2_F555W is not the line of one ion" in r.stderr
    run(tmp_path, "--emission", "--params", "images.param", "--file", plain)

    with_keys = sorted(os.listdir(tmp_path / "with"))
    without = sorted(os.listdir(tmp_path / "without"))
    names = ["line_image_%s%s.dat" % (line, view)
             for line in ("Halpha", "OIII_5007", "WFC2_F555W")
             for view in ("", "_view1")]
    cubes = ["line_image_%s_cube%s.dat" % (line, view)
             for line in ("Halpha", "OIII_5007") for view in ("", "_view1")]
    assert without == sorted(names)
    assert with_keys == sorted(names + cubes)
    # the keys change none of the other outputs
    for name in names:
        assert open(str(tmp_path / "with" / name), "rb").read() == \
            open(str(tmp_path / "without" / name), "rb").read(), name
    a, b = hdf5_mini.read(snapshot), hdf5_mini.read(plain)
    assert sorted(a["/PartType0"].members) == sorted(b["/PartType0"].members)
    for name, node in b["/PartType0"].members.items():
        assert np.array_equal(a["/PartType0/" + name].data, node.data), name
    used = open(str(tmp_path / "images.param.used-values")).read()
    assert "velocity" not in used and "expansion" not in used
    used = open(str(tmp_path / "cubes.param.used-values")).read()
    assert "velocity channels: 8" in used
    assert "velocity maximum: 300000 m s^-1" in used

    # +-300 km/s covers u +- 6 b of every cell (|u| < 35 km/s, b < 20 km/s up
    # to 24000 K for hydrogen): the channels sum to the image as in case 4 of
    # test_gpu_line_cube.py; a ray crosses at most 3 NCELL cells
    allowed = (nchan + 8 * 3 * NCELL) * EPS
    for line in ("Halpha", "OIII_5007"):
        for view in ("", "_view1"):
            cube = np.fromfile(str(tmp_path / "with" / (
                "line_image_%s_cube%s.dat" % (line, view))))
            assert cube.shape == (nchan * nx * ny,)
            cube = cube.reshape(nchan, nx, ny)
            image = np.fromfile(str(tmp_path / "with" / (
                "line_image_%s%s.dat" % (line, view)))).reshape(nx, ny)
            lit = image > 0.
            assert lit.sum() > 0.3 * nx * ny
            total = cube.sum(axis=0)
            assert not total[~lit].any()
            err = (np.abs(total - image)[lit] / image[lit]).max()
            print(line, view, "worst", err, "allowed", allowed)
            assert err <= allowed
            # the line is resolved: the expansion and the thermal width put
            # it into the middle channels, more than one of them
            assert (cube.sum(axis=(1, 2)) > 0.).sum() >= 2
            assert not cube[0].any() and not cube[-1].any()

    # the lexington run writes no velocities: Snapshot names what it misses
    (tmp_path / "snapshot.param").write_text(
        switches + block % (nx, ny, tmp_path / "with") +
        cube_keys.split("  velocity field type")[0] +
        "  velocity field type: Snapshot\n")
    r = run(tmp_path, "--emission", "--params", "snapshot.param", "--file",
            plain, fails=True)
    assert "/PartType0/Velocities" in r.stderr, r.stderr
