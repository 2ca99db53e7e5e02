"""Emission-line images without a GPU: the CPU restatement
(tests/support/line_image_reference.c) against numpy and against analytic
values - it is what the GPU tests compare the kernels with, so it has to be
right on its own -, the exported symbols, and the driver's refusal of a bad
EmissionImages block."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_image_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMI_GPU = os.path.join(ROOT, "cmacionize_amd", "cmi-gpu")
FOURPI = 4. * np.pi
HALF = 0.5 * np.pi

BOX = L.Box((-1., 0.5, 2.), (3., 2., 2.5), (12, 8, 10))
OBLIQUE = [(0.7, 0.3), (2.1, 4.0), (1.2, -2.5), (np.radians(89.7), 0.4)]


def random_field(box, seed, nfields=1):
    rng = np.random.default_rng(seed)
    return 10. ** rng.uniform(-2., 1., (nfields, box.n))


def test_axis_views_are_column_sums():
    """(a) theta = 0: image x = +y, image y = -x, one pixel per (x, y)
    column through the cell centres: sum_z j dz / 4 pi. Likewise along x
    (theta = 90 deg, phi = 0: image x = +y, image y = +z) and along y (phi =
    90 deg: image x = -x, image y = +z). cos 90 deg is 6e-17, not 0: the ray
    drifts by that much, so rtol 1e-12 and not equality."""
    box = BOX
    j = random_field(box, 1)[0]
    cube = j.reshape(tuple(box.ncell))
    dx, dy, dz = box.cellside
    a, s, nc = box.anchor, box.sides, box.ncell
    img = L.render(box, j, 0., 0., nc[1], nc[0], (a[1], -(a[0] + s[0])),
                   (s[1], s[0]))[0]
    want = (cube.sum(axis=2) * dz / FOURPI)[::-1, :].T
    assert np.allclose(img, want, rtol=1e-12, atol=0.)
    assert L.last_crossings == box.n
    img = L.render(box, j, HALF, 0., nc[1], nc[2], (a[1], a[2]),
                   (s[1], s[2]))[0]
    want = cube.sum(axis=0) * dx / FOURPI
    assert np.allclose(img, want, rtol=1e-12, atol=0.)
    img = L.render(box, j, HALF, HALF, nc[0], nc[2], (-(a[0] + s[0]), a[2]),
                   (s[0], s[2]))[0]
    want = (cube.sum(axis=1) * dy / FOURPI)[::-1, :]
    assert np.allclose(img, want, rtol=1e-12, atol=0.)


@pytest.mark.parametrize("theta,phi", OBLIQUE)
def test_uniform_box_is_the_chord(theta, phi):
    """(b) every pixel of a uniform box is j chord / 4 pi, or (j / 4 pi k)
    (1 - exp(-k chord)) with dust; the chord from numpy's own slab test"""
    box = BOX
    j, k = 3.7, 0.9
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    # a margin, so that every view has rays that miss
    anchor, sides = anchor - 0.1 * sides, 1.2 * sides
    nx, ny = 37, 29
    xy = L.sample_coordinates(nx, ny, anchor, sides)[:, :, 0, 0, :]
    chord = L.chords(box, theta, phi, xy.reshape(-1, 2)).reshape(nx, ny)
    assert (chord > 0.).sum() > 300 and (chord == 0.).sum() > 20
    img = L.render(box, np.full(box.n, j), theta, phi, nx, ny, anchor,
                   sides)[0]
    assert np.allclose(img, j * chord / FOURPI, rtol=1e-12, atol=0.)
    assert not img[chord == 0.].any()
    img = L.render(box, np.full(box.n, j), theta, phi, nx, ny, anchor, sides,
                   extinction=np.full(box.n, k))[0]
    want = j / (FOURPI * k) * -np.expm1(-k * chord)
    assert np.allclose(img, want, rtol=1e-12, atol=0.)


def test_probe_steps_add_up_to_the_chord():
    """(c) sum of ds = t_out - t_in for every ray; a miss has no steps. The
    1e-12 is relative to the numbers the difference is taken of: t_in and
    t_out carry a rounding error of eps |t| each, whatever is left of them
    after the subtraction (a ray that clips an edge has a chord far smaller
    than either)."""
    box = BOX
    rng = np.random.default_rng(5)
    nmax = int(box.ncell.sum()) + 3
    for theta, phi in OBLIQUE + [(0., 0.), (HALF, 0.), (HALF, HALF)]:
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        xy = anchor + sides * rng.uniform(-0.1, 1.1, (4000, 2))
        rows = L.probe(box, theta, phi, xy, nmax)
        steps = rows[:, 2].astype(int)
        miss = steps == 0
        assert miss.sum() > 50 and (~miss).sum() > 2000
        assert np.isnan(rows[miss, 0]).all() and np.isnan(rows[miss, 1]).all()
        assert not rows[miss, 3:].any()
        assert steps.max() <= nmax - 3
        ds = rows[:, 3 + nmax:]
        hit = rows[~miss]
        total = ds[~miss].sum(axis=1)
        scale = np.maximum(np.abs(hit[:, 0]), np.abs(hit[:, 1]))
        assert (np.abs(total - (hit[:, 1] - hit[:, 0])) <= 1e-12 * scale).all()
        # and the independent slab test agrees on who misses and how long
        chord = L.chords(box, theta, phi, xy)
        assert np.array_equal(chord == 0., miss)
        assert (np.abs(total - chord[~miss]) <= 1e-12 * scale).all()
        # every cell of a ray is a cell of the grid, none twice
        cells = rows[:, 3:3 + nmax].astype(np.int64)
        for r in np.flatnonzero(~miss)[:200]:
            c = cells[r, :steps[r]]
            assert (c >= 0).all() and (c < box.n).all()
            assert len(set(c.tolist())) == len(c)


FLUX_VIEW = (1.1, 0.6)


def flux_error(s):
    box = L.Box((0., 0., 0.), (1., 1., 1.), (16, 16, 16))
    j = random_field(box, 9)[0]
    theta, phi = FLUX_VIEW
    anchor, sides = L.bounding_rectangle(box, theta, phi)
    nx = ny = 64
    img = L.render(box, j, theta, phi, nx, ny, anchor, sides, s)[0]
    flux = img.sum() * (sides[0] / nx) * (sides[1] / ny)
    want = j.sum() * np.prod(box.cellside) / FOURPI
    return abs(flux - want) / want


def test_a_ray_that_is_not_finite_misses():
    """A NaN or infinite image coordinate goes through fmax / fmin and would
    leave the slab test with t_in = -inf, t_out = +inf: such a ray is a miss
    (the NaN row, no steps), for every view, and an image sample there is 0."""
    bad = [[np.nan, 0.], [0., np.nan], [np.nan, np.nan], [np.inf, 0.],
           [0., -np.inf], [np.inf, np.nan]]
    for theta, phi in OBLIQUE + [(0., 0.), (HALF, 0.), (HALF, HALF)]:
        rows = L.probe(BOX, theta, phi, bad, 4)
        assert np.isnan(rows[:, :2]).all()
        assert not rows[:, 2:].any()
    img = L.render(BOX, np.ones((1, BOX.n)), 0.7, 0.3, 2, 2, (np.nan, 0.),
                   (1., 1.))
    assert not img.any()


def test_flux_is_conserved_without_dust():
    """(d) sum over pixels of I x pixel area against (1 / 4 pi) sum over
    cells of j V, for a random field (3 decades) on 16^3 cells, view theta =
    1.1, phi = 0.6, 64 x 64 pixels over the bounding rectangle. The image
    integrates the projected emission with the midpoint rule over s^2 samples
    per pixel; its error is not derivable, so it is measured with the
    restatement alone:
        s = 1: 1.09e-03   s = 2: 1.88e-04   s = 4: 1.90e-04   s = 8: 4.07e-07
    (not monotonic: the signed error changes sign between 2 and 8). The
    assertion for s = 4 is twice its measured value."""
    errors = {s: flux_error(s) for s in (1, 2, 4, 8)}
    print("flux errors:", errors)
    assert errors[4] < 2. * 1.90e-04
    assert errors[8] < errors[1] and errors[4] < errors[1]


def test_library_exports_the_line_image_symbols():
    """(e)"""
    from cmacionize_amd import engine
    names = ["cmi_gpu_render_line_images", "cmi_gpu_render_field_images",
             "cmi_gpu_line_image_probe"]
    lib = C.CDLL(engine.LIB_PATH)
    for name in names:
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    for name in ("render_line_images", "render_field_images",
                 "line_image_probe"):
        assert callable(getattr(engine.GpuEngine, name))


@pytest.mark.parametrize("block,message", [
    ("  type: JPEG\n", "EmissionImages:type"),
    ("  image width: 0\n", "image width"),
    ("  supersampling: 9\n", "supersampling"),
    ("  dust cross section per hydrogen: -1. m^2\n", "cross section"),
])
def test_driver_refuses_a_bad_block_first(tmp_path, block, message):
    """(f) a bad EmissionImages block ends `cmi-gpu --emission` with a
    message before the snapshot is opened or a device touched: the snapshot
    named here does not exist, and that is not what the run complains of"""
    params = tmp_path / "lines.param"
    params.write_text("EmissivityValues:\n  Halpha: true\n"
                      "EmissionImages:\n" + block)
    r = subprocess.run([CMI_GPU, "--emission", "--params", str(params),
                        "--file", str(tmp_path / "nowhere.hdf5")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(str(params) + ".used-values")


def test_driver_without_the_block_reads_none_of_its_keys(tmp_path):
    """the used-values dump of a parameter file without the block does not
    mention it (a key that is read appears there with its default)"""
    params = tmp_path / "lines.param"
    params.write_text("EmissivityValues:\n  Halpha: true\n")
    r = subprocess.run([CMI_GPU, "--emission", "--params", str(params),
                        "--file", str(tmp_path / "nowhere.hdf5")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "Could not open" in r.stderr
    used = open(str(params) + ".used-values").read()
    assert "Halpha: true" in used
    assert "EmissionImages" not in used and "image" not in used
