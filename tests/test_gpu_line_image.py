"""Emission-line images on the device (cmi_gpu_render_line_images,
cmi_gpu_render_field_images, cmi_gpu_line_image_probe) against the CPU
restatement (tests/support/line_image_reference.c, checked on its own in
test_line_image_host.py), against analytic values and against themselves."""
import ctypes as C

import numpy as np
import pytest

import line_image_lib as L
from test_gpu_emissivity import random_state
from test_gpu_physics import lexington_engine

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
HALF = 0.5 * np.pi
GRAZING = np.radians(89.7)
BOX = L.Box((-1., 0.5, 2.), (3., 2., 2.5), (24, 16, 20))
EINVAL, ESTATE = 1, 3  # include/cmi_gpu.h
VIEWS = [(0., 0.), (HALF, 0.), (HALF, HALF), (0.7, 0.3), (2.1, 4.0),
         (GRAZING, 0.4)]


def plain_engine(box):
    from cmacionize_amd import GpuEngine
    return GpuEngine(tuple(int(n) for n in box.ncell), tuple(box.anchor),
                     tuple(box.sides), (0, 0, 0), device=0)


def view_rays(box, theta, phi, rng, nrandom):
    """image coordinates: random ones over the bounding rectangle and a
    margin around it (those miss), the box's corners, and vertices of the
    grid (rays through corners and edges of cells)"""
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    _, ex, ey = L.axes(theta, phi)
    xy = [anchor + sides * rng.uniform(-0.15, 1.15, (nrandom, 2))]
    idx = np.stack(np.meshgrid(*[np.arange(0, n + 1, 4) for n in box.ncell],
                               indexing="ij"), axis=-1).reshape(-1, 3)
    vertices = box.anchor + idx * box.cellside
    xy.append(np.stack([vertices @ ex, vertices @ ey], axis=1))
    return np.concatenate(xy)


def test_probe_is_the_restatement_ray_for_ray():
    """Case 1: cells, step counts, path lengths and the box entry / exit
    parameters of ~2e4 rays over six views - equal, not close: the device
    does the restatement's IEEE operations (no contraction on either side)."""
    eng = plain_engine(BOX)
    rng = np.random.default_rng(3)
    nmax = int(BOX.ncell.sum()) + 3
    nrays = 0
    for theta, phi in VIEWS:
        xy = view_rays(BOX, theta, phi, rng, 3000)
        got = eng.line_image_probe(theta, phi, xy, nmax)
        want = L.probe(BOX, theta, phi, xy, nmax)
        steps = want[:, 2].astype(int)
        print("view", theta, phi, "rays", len(xy), "misses",
              int((steps == 0).sum()), "longest", steps.max())
        assert (steps == 0).sum() > 100 and (steps > 0).sum() > 1000
        assert steps.max() <= nmax - 3
        assert np.array_equal(got[:, 2], want[:, 2])
        assert np.array_equal(got[:, 3:3 + nmax], want[:, 3:3 + nmax])
        assert np.array_equal(got[:, 3 + nmax:], want[:, 3 + nmax:])
        assert np.array_equal(got[:, :2], want[:, :2], equal_nan=True)
        nrays += len(xy)
    assert nrays > 19000
    eng.close()


def longest_ray(box, theta, phi, nx, ny, anchor, sides, s):
    xy = L.sample_coordinates(nx, ny, anchor, sides, s).reshape(-1, 2)
    return int(L.probe(box, theta, phi, xy, 0)[:, 2].max())


@pytest.mark.parametrize("nfields", [3, 9])
def test_field_images_match_the_restatement(nfields):
    """Case 2: random positive fields, one and two batches. Without
    extinction rtol 1e-13 (same terms in the same order; whether the images
    are equal to the bit is printed); with random extinction 8 eps x the longest
    ray of the view in steps - one exp and one expm1 of a few ulp each per
    step, compounding through I exp(-dtau) + ..."""
    eng = plain_engine(BOX)
    rng = np.random.default_rng(17 + nfields)
    fields = 10. ** rng.uniform(-2., 1., (nfields, BOX.n))
    # optical depths per cell around 0.1, some cells without dust
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n)
    k[rng.uniform(size=BOX.n) < 0.1] = 0.
    for (theta, phi), s in zip(VIEWS, (1, 2, 1, 3, 1, 2)):
        anchor, sides = L.bounding_rectangle(BOX, theta, phi)
        nx, ny = 45, 38
        want = L.render(BOX, fields, theta, phi, nx, ny, anchor, sides, s)
        got = eng.render_field_images(fields, theta, phi, nx, ny, anchor,
                                      sides, s)
        assert got.shape == want.shape == (nfields, nx, ny)
        assert (want > 0.).sum() > 0.3 * want.size
        print("view", theta, phi, "s", s, "no dust: equal",
              np.array_equal(got, want))
        assert np.allclose(got, want, rtol=1e-13, atol=0.)
        nsteps = longest_ray(BOX, theta, phi, nx, ny, anchor, sides, s)
        rtol = 8. * EPS * nsteps
        want = L.render(BOX, fields, theta, phi, nx, ny, anchor, sides, s,
                        extinction=k)
        got = eng.render_field_images(fields, theta, phi, nx, ny, anchor,
                                      sides, s, extinction=k)
        err = np.abs(got - want) / np.maximum(want, 1e-300)
        print("  dust: longest ray", nsteps, "rtol", rtol, "worst",
              err[want > 0.].max())
        assert np.array_equal(got == 0., want == 0.)
        assert (err[want > 0.] <= rtol).all()
    eng.close()


@pytest.mark.parametrize("s, nx", [(8, 16384 + 50), (1, (1 << 20) + 50)])
def test_more_pixel_rows_than_one_launch_takes(s, nx):
    """Case 2, the chunks of pixel rows: a launch takes 2^22 sample rays
    (CMI_LINE_IMAGE_LAUNCH_SAMPLES), with ny = 4 that is 16384 pixel rows at
    s = 8 and 2^20 at s = 1, and a second launch marches the last 50 - through
    the sample buffer and the reduction at s = 8, straight into the image at
    its row offset at s = 1. Two fields, no extinction, rtol 1e-13 as in Case
    2, on the middle of the oblique view's rectangle so that every pixel is
    lit, the last chunk's among them."""
    ny = 4
    rows = (1 << 22) // (ny * s * s)
    assert nx == rows + 50
    eng = plain_engine(BOX)
    rng = np.random.default_rng(23 + s)
    fields = 10. ** rng.uniform(-2., 1., (2, BOX.n))
    theta, phi = 0.7, 0.3
    anchor, sides = L.bounding_rectangle(BOX, theta, phi)
    anchor, sides = anchor + 0.25 * sides, 0.5 * sides
    want = L.render(BOX, fields, theta, phi, nx, ny, anchor, sides, s)
    got = eng.render_field_images(fields, theta, phi, nx, ny, anchor, sides, s)
    assert got.shape == want.shape == (2, nx, ny)
    assert (want > 0.).all()
    assert (got[:, rows:] > 0.).any()
    print("s", s, "nx", nx, "equal", np.array_equal(got, want))
    assert np.allclose(got, want, rtol=1e-13, atol=0.)
    eng.close()


LEX_LINES = ["HAlpha", "HBeta", "OIII_5007", "NII_6584", "OII_3727",
             "SII_6725", "NeIII_3869", "SIII_9405", "HeI_5876", "CII_158mu",
             "WFC2_F555W"]
DUST_SIGMA = 2.e-27  # m^2 per H: optical depths of order one across the box


def lexington_box(ncell):
    import oracle_lib as o
    return L.Box((-5. * o.PC,) * 3, (10. * o.PC,) * 3, (ncell,) * 3)


def test_line_images_end_to_end(oracle):
    """Case 3: the random lexington state of test_gpu_emissivity.py: device
    emissivities, records and march against the restatement fed with the
    oracle's emissivities. rtol 2e-10: that file's 1e-10 for an emissivity,
    carried through a sum of positive terms, plus the march's own bound of
    case 2 (8 eps x steps, ~1e-13). Without and with dust."""
    from cmacionize_amd import engine as E
    ncell = 12
    sim = oracle.lexington_simulation(ncell)
    density, temperature, x = random_state(ncell, 7)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    box = lexington_box(ncell)
    n = ncell ** 3
    ref = np.array([oracle.emissivities(sim.model, density[c], temperature[c],
                                        x[:, c]) for c in range(n)]).T
    dark = ~((x[0] < 0.2) & (temperature > 3000.))
    assert dark.sum() > 10 and not ref[:, dark].any()
    idx = [E.EMISSION_LINES.index(name) for name in LEX_LINES]
    for (theta, phi), s in (((0.7, 0.3), 1), ((GRAZING, 0.4), 2)):
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        nx, ny = 40, 33
        for sigma in (0., DUST_SIGMA):
            got = eng.render_line_images(LEX_LINES, theta, phi, nx, ny,
                                         anchor, sides, s, sigma)
            assert list(got) == LEX_LINES
            want = L.render(box, ref[idx], theta, phi, nx, ny, anchor, sides,
                            s, extinction=density * sigma if sigma else None)
            for k, name in enumerate(LEX_LINES):
                assert got[name].shape == (nx, ny)
                lit = want[k] > 0.
                assert lit.sum() > 0.3 * nx * ny
                assert not got[name][~lit].any(), name
                err = np.abs(got[name] - want[k])[lit] / want[k][lit]
                print(name, "sigma", sigma, "worst", err.max())
                assert err.max() < 2.e-10, (name, sigma, err.max())
            if sigma:
                plain = eng.render_line_images(["HAlpha"], theta, phi, nx, ny,
                                               anchor, sides, s)["HAlpha"]
                assert (got["HAlpha"] <= plain).all()
                assert got["HAlpha"].sum() < 0.9 * plain.sum()
    # dark cells (x_H >= 0.2 or T <= 3000 K) contribute nothing
    x_dark = x.copy()
    x_dark[0] = np.where(np.arange(n) % 2, 0.2, 0.5)
    t_dark = temperature.copy()
    eng.upload_cells(density, t_dark, x_dark)
    anchor, sides = L.bounding_rectangle(box, 0.7, 0.3)
    for img in eng.render_line_images(None, 0.7, 0.3, 20, 20, anchor, sides,
                                      1, DUST_SIGMA).values():
        assert not img.any()
    x_cold = x.copy()
    x_cold[0] = 1.e-3
    eng.upload_cells(density, np.full(n, 3000.), x_cold)
    for img in eng.render_line_images(["HAlpha", "OIII_5007"], 0.7, 0.3, 20,
                                      20, anchor, sides).values():
        assert not img.any()
    eng.close()


def test_selected_lines_repeats_and_supersampling():
    """Case 4, first three: selected lines in any order are the lines of an
    all-lines render, bit for bit (other batches, other record sizes); two
    identical calls give identical bits; supersampling 1 and 3 of a uniform
    box both meet the analytic value."""
    from cmacionize_amd import engine as E
    ncell = 10
    density, temperature, x = random_state(ncell, 23)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    box = lexington_box(ncell)
    theta, phi = 1.2, -2.5
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    args = (theta, phi, 31, 27, anchor, sides, 2, DUST_SIGMA)
    everything = eng.render_line_images(None, *args)
    assert list(everything) == E.EMISSION_LINES
    again = eng.render_line_images(None, *args)
    for name in E.EMISSION_LINES:
        assert np.array_equal(everything[name], again[name]), name
    for some in (["WFC2_F675W", "HAlpha", "OIII_5007"], ["SIV_10mu"],
                 E.EMISSION_LINES[::-1][:9], ["HBeta", "HBeta"]):
        got = eng.render_line_images(some, *args)
        for name in some:
            assert np.array_equal(got[name], everything[name]), name
    eng.close()

    eng = plain_engine(BOX)
    j, k = 3.7, 0.9
    for theta, phi in ((0.7, 0.3), (GRAZING, 0.4)):
        anchor, sides = L.bounding_rectangle(BOX, theta, phi)
        anchor, sides = anchor - 0.1 * sides, 1.2 * sides
        nx, ny = 37, 29
        for s in (1, 3):
            xy = L.sample_coordinates(nx, ny, anchor, sides, s)
            chord = L.chords(BOX, theta, phi, xy.reshape(-1, 2))
            chord = chord.reshape(nx, ny, s * s)
            got = eng.render_field_images(np.full(BOX.n, j), theta, phi, nx,
                                          ny, anchor, sides, s)[0]
            want = (j * chord / (4. * np.pi)).mean(axis=2)
            assert np.allclose(got, want, rtol=1e-12, atol=0.)
            got = eng.render_field_images(np.full(BOX.n, j), theta, phi, nx,
                                          ny, anchor, sides, s,
                                          extinction=np.full(BOX.n, k))[0]
            want = (j / (4. * np.pi * k) * -np.expm1(-k * chord)).mean(axis=2)
            assert np.allclose(got, want, rtol=1e-12, atol=0.)
    eng.close()


def test_rotated_state_rotated_view():
    """Case 4, last: the state turned by 90 degrees about z and seen from
    phi + 90 degrees is the same image, pixel for pixel, to rtol 1e-12 (sin
    and cos of phi + pi / 2 are not those of phi swapped, to the last bit)."""
    ncell = 14
    box = L.Box((-2., -2., -1.), (4., 4., 3.), (ncell, ncell, 9))
    eng = plain_engine(box)
    rng = np.random.default_rng(31)
    shape = tuple(box.ncell)
    fields = 10. ** rng.uniform(-2., 1., (2,) + shape)
    k = 10. ** rng.uniform(-1.5, 0., shape)
    # cell (i, j) goes to (N - 1 - j, i): turned[a, b] = cube[b, N - 1 - a]
    turn = lambda cube: np.ascontiguousarray(
        np.swapaxes(cube, -3, -2)[..., ::-1, :, :])
    assert turn(fields)[0, ncell - 1 - 3, 5, 2] == fields[0, 5, 3, 2]
    for theta, phi in ((0.7, 0.3), (2.1, 4.0)):
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        for ext in (None, k):
            a = eng.render_field_images(fields, theta, phi, 33, 29, anchor,
                                        sides, 2, extinction=ext)
            b = eng.render_field_images(
                turn(fields), theta, phi + HALF, 33, 29, anchor, sides, 2,
                extinction=None if ext is None else turn(ext))
            assert (a > 0.).sum() > 0.3 * a.size
            assert np.allclose(a, b, rtol=1e-12, atol=0.)
    eng.close()


def test_bad_arguments_are_refused_and_the_engine_lives():
    """Case 5"""
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    lib = E.load_library()
    eng = lexington_engine(4)
    anchor, sides = (C.c_double * 2)(-1., -1.), (C.c_double * 2)(2., 2.)
    out = (C.c_double * (42 * 64))()
    line = (C.c_int32 * 2)(0, 1)

    def lines(nlines=1, theta=0.3, phi=0.2, nx=4, ny=4, a=anchor, s=sides,
              ss=1, sigma=0.):
        return lib.cmi_gpu_render_line_images(eng._h, nlines, line, theta,
                                              phi, nx, ny, a, s, ss, sigma,
                                              out)

    assert lines() == ESTATE
    assert b"cell data" in lib.cmi_gpu_last_error()
    eng.upload_cells(np.full(64, 1e8), np.full(64, 8000.),
                     np.full((14, 64), 1e-3))
    einval = EINVAL
    assert lines(nx=0) == einval and lines(ny=-3) == einval
    assert lines(nx=1 << 15, ny=(1 << 13) + 1) == einval
    assert b"2^28" in lib.cmi_gpu_last_error()
    assert lines(ss=0) == einval and lines(ss=9) == einval
    assert b"supersampling" in lib.cmi_gpu_last_error()
    assert lines(nx=1 << 28, ny=1, ss=8) == einval  # 2^31 samples in a row
    assert lines(sigma=-1.e-30) == einval
    assert lines(s=(C.c_double * 2)(2., 0.)) == einval
    assert lines(s=(C.c_double * 2)(-2., 1.)) == einval
    assert lines(nlines=0) == einval and lines(nlines=43) == einval
    line[1] = 42
    assert lines(nlines=2) == einval
    assert b"no emission line 42" in lib.cmi_gpu_last_error()
    line[1] = -1
    assert lines(nlines=2) == einval
    line[1] = 1
    assert lines(nlines=2) == 0
    xy = (C.c_double * 2)(0., 0.)
    row = (C.c_double * 5)()
    assert lib.cmi_gpu_line_image_probe(eng._h, 0.3, 0.2, 1, xy, -1,
                                        row) == einval
    assert lib.cmi_gpu_line_image_probe(eng._h, 0.3, 0.2, 1, xy, 1, row) == 0
    for bad in (float("nan"), float("inf")):
        for which in (0, 1):
            xy[which] = bad
            assert lib.cmi_gpu_line_image_probe(eng._h, 0.3, 0.2, 1, xy, 1,
                                                row) == einval
            assert b"not finite" in lib.cmi_gpu_last_error()
            xy[which] = 0.
    assert lib.cmi_gpu_line_image_probe(eng._h, 0.3, 0.2, 1, xy, 1, row) == 0
    field = (C.c_double * 64)(*([1.] * 64))
    assert lib.cmi_gpu_render_field_images(eng._h, 0, field, 0.3, 0.2, 4, 4,
                                           anchor, sides, 1, None,
                                           out) == einval
    assert lib.cmi_gpu_render_field_images(eng._h, 1, field, 0.3, 0.2, 4, 4,
                                           anchor, sides, 1, None, out) == 0
    # the engine still computes
    assert eng.compute_emissivities(["HAlpha"])["HAlpha"].min() > 0.
    eng.close()

    periodic = GpuEngine((4, 4, 4), (0., 0., 0.), (1., 1., 1.), (1, 0, 0),
                         device=0)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.render_field_images(np.ones(64), 0.3, 0.2, 4, 4, (-1., -1.),
                                     (2., 2.))
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.line_image_probe(0.3, 0.2, [[0., 0.]], 4)
    periodic.close()
    block = GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                      device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    with pytest.raises(E.EngineError, match="decomposed"):
        block.render_field_images(np.ones(64), 0.3, 0.2, 4, 4, (-1., -1.),
                                  (2., 2.))
    assert block.n == 64
    block.close()


# the reference's names of the lines in parameter files and snapshots
FILE_NAMES = {"Halpha": "HAlpha", "Hbeta": "HBeta", "OIII_5007": "OIII_5007",
              "NII_6584": "NII_6584"}


def test_driver_writes_the_images_of_a_snapshot(tmp_path):
    """Case 6: `cmi-gpu --emission` with an EmissionImages block on the
    snapshot of a short lexington run: each .dat is render_line_images of the
    same state, equal; the PGM variant has its header and size; the datasets
    the mode adds to the snapshot are what it adds without the block."""
    import os
    import shutil
    import subprocess
    import hdf5_mini
    import oracle_lib as o
    from cmacionize_amd import engine as E
    root = L.ROOT
    exe = os.path.join(root, "cmacionize_amd", "cmi-gpu")
    bench = os.path.join(root, "benchmarks")
    ncell = 14
    text = open(os.path.join(bench, "lexingtonHII40.param")).read()
    text = text.replace("[64, 64, 64]", "[%d, %d, %d]" % ((ncell,) * 3))
    text = text.replace("number of photons: 1e8", "number of photons: 30000")
    text = text.replace("number of iterations: 20", "number of iterations: 6")
    text = text.replace("NumberDensity: 0", "NumberDensity: 1")
    shutil.copy(os.path.join(bench, "lexingtonHII40.yml"), tmp_path)
    (tmp_path / "run.param").write_text(text)
    r = subprocess.run([exe, "--params", "run.param"], capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    snapshot = str(tmp_path / "lexingtonHII40_006.hdf5")
    plain = str(tmp_path / "plain.hdf5")
    shutil.copy(snapshot, plain)

    theta, phi, nx, ny, s, sigma = 1.05, 0.5, 48, 40, 2, 2.e-27
    anchor, sides = (-1.75e17, -1.5e17), (3.5e17, 3.25e17)
    switches = "EmissivityValues:\n" + "".join(
        "  %s: true\n" % name for name in FILE_NAMES)
    block = ("EmissionImages:\n  view theta: %r radians\n"
             "  view phi: %r radians\n  image width: %d\n  image height: %d\n"
             "  anchor x: %r m\n  anchor y: %r m\n  sides x: %r m\n"
             "  sides y: %r m\n  supersampling: %d\n"
             "  dust cross section per hydrogen: %r m^2\n"
             "  filename prefix: map\n  output folder: %s\n" %
             (theta, phi, nx, ny, anchor[0], anchor[1], sides[0], sides[1], s,
              sigma, str(tmp_path)))
    (tmp_path / "images.param").write_text(switches + block)
    (tmp_path / "lines.param").write_text(switches)
    r = subprocess.run([exe, "--emission", "--params", "images.param",
                        "--file", snapshot], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--emission", "--params", "lines.param",
                        "--file", plain], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert not [n for n in os.listdir(tmp_path) if n.startswith("line_image")]
    # the snapshot got the same datasets either way, in the file's order
    with_images, without = hdf5_mini.read(snapshot), hdf5_mini.read(plain)
    assert sorted(with_images["/PartType0"].members) == \
        sorted(without["/PartType0"].members)
    for name, node in without["/PartType0"].members.items():
        assert np.array_equal(with_images["/PartType0/" + name].data,
                              node.data), name
    used = open(str(tmp_path / "images.param.used-values")).read()
    assert "EmissionImages:" in used and "type: BinaryArray" in used
    assert "EmissionImages" not in \
        open(str(tmp_path / "lines.param.used-values")).read()

    # the same state on an engine of our own, every cell where its
    # coordinates put it
    f = without
    ions = ["H", "He", "C+", "C++", "N", "N+", "N++", "O", "O+", "Ne", "Ne+",
            "S+", "S++", "S+++"]
    unit_length = 0.01 * float(np.ravel(
        f["/Units"].attrs["Unit length in cgs (U_L)"])[0])
    box_sides = 10. * o.PC
    mid = f["/PartType0/Coordinates"].data.reshape(-1, 3) * unit_length
    idx = np.floor(ncell * mid / box_sides).astype(np.int64)
    cell = (idx[:, 0] * ncell + idx[:, 1]) * ncell + idx[:, 2]
    assert sorted(cell) == list(range(ncell ** 3))

    def placed(values):
        out = np.empty_like(values)
        out[..., cell] = values
        return out

    unit_n = 1. / unit_length ** 3
    eng = lexington_engine(ncell)
    eng.upload_cells(
        placed(f["/PartType0/NumberDensity"].data * unit_n),
        placed(f["/PartType0/Temperature"].data * float(np.ravel(
            f["/Units"].attrs["Unit temperature in cgs (U_T)"])[0])),
        placed(np.array([f["/PartType0/NeutralFraction" + i].data
                         for i in ions])))
    want = eng.render_line_images(list(FILE_NAMES.values()), theta, phi, nx,
                                  ny, anchor, sides, s, sigma)
    for file_name, name in FILE_NAMES.items():
        got = np.fromfile(str(tmp_path / ("map_%s.dat" % file_name)))
        assert got.shape == (nx * ny,)
        assert got.max() > 0.
        assert np.array_equal(got.reshape(nx, ny), want[name]), name
    eng.close()

    # PGM, default rectangle and size
    (tmp_path / "pgm.param").write_text(
        switches + "EmissionImages:\n  view theta: 60. degrees\n"
        "  type: PGM\n  image width: 30\n")
    r = subprocess.run([exe, "--emission", "--params", "pgm.param", "--file",
                        snapshot], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    for file_name in FILE_NAMES:
        words = open(str(tmp_path / ("line_image_%s.pgm" % file_name))).read()
        words = words.split()
        assert words[:4] == ["P2", "30", "200", "255"]
        pixels = np.array(words[4:], dtype=int)
        assert pixels.shape == (30 * 200,)
        assert pixels.min() == 0 and pixels.max() == 255
