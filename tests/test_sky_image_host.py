"""Sky maps without a GPU: the CPU restatement
(tests/support/sky_image_reference.c) against closed forms, against the
plane-parallel restatement (tests/support/line_image_reference.c) and on the
edge cases of the start cell - it is what the GPU tests compare the kernels
with, so it has to be right on its own -, the map's directions and solid
angles, the exported symbols, and the driver's refusal of a bad
EmissionSkyMaps block."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_image_lib as L
import sky_image_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMI_GPU = os.path.join(ROOT, "cmacionize_amd", "cmi-gpu")
FOURPI = 4. * np.pi
HALF = 0.5 * np.pi
EPS = np.finfo(np.float64).eps

# unequal cell sides (0.25, 0.2, 0.17857...), anchor away from the origin
BOX = S.Box((-1., 0.5, 2.), (3., 2., 2.5), (12, 10, 14))
# the same grid with cell sides 0.25, 0.125, 0.5: every wall is a double
EXACT = S.Box((-1., 0.5, 2.), (3., 1.25, 7.), (12, 10, 14))
INSIDE = (0.3, 1.1, 3.4)
AXES = np.array([[1., 0., 0.], [-1., 0., 0.], [0., 1., 0.], [0., -1., 0.],
                 [0., 0., 1.], [0., 0., -1.]])


def chord_directions(seed):
    return np.concatenate([S.random_directions(np.random.default_rng(seed),
                                               3000), AXES])


def test_uniform_box_without_dust_is_the_chord():
    """1: uniform j, observer inside: every ray is (j / 4 pi) L, L the
    distance to the wall in closed form. rtol 1e-12: at most ~40 additions of
    positive terms."""
    j = 3.7
    d = chord_directions(1)
    length = S.wall_distance(BOX, INSIDE, d)
    assert length.min() > 0. and np.isfinite(length).all()
    got = S.render(BOX, np.full(BOX.n, j), INSIDE, d)[0]
    assert np.allclose(got, j / FOURPI * length, rtol=1e-12, atol=0.)
    assert S.last_crossings > len(d)


def test_uniform_box_with_dust_is_the_attenuated_chord():
    """2: uniform k > 0: (j / 4 pi k) (1 - exp(-k L))"""
    j, k = 3.7, 0.9
    d = chord_directions(2)
    length = S.wall_distance(BOX, INSIDE, d)
    got = S.render(BOX, np.full(BOX.n, j), INSIDE, d,
                   extinction=np.full(BOX.n, k))[0]
    want = j / (FOURPI * k) * -np.expm1(-k * length)
    assert np.allclose(got, want, rtol=1e-12, atol=0.)


def unravel(box, cells):
    return np.stack(np.unravel_index(cells, tuple(box.ncell)), axis=-1)


def test_probe_steps_add_up_and_cells_are_neighbours():
    """3: sum of ds = t_out - t_start (1e-12 relative to the larger of the
    two, which carry a rounding error of eps |t| each), and consecutive cells
    of a ray are face, edge or corner neighbours; from inside and from
    outside, where part of the rays miss"""
    rng = np.random.default_rng(3)
    nmax = int(BOX.ncell.sum()) + 3
    for origin, some_miss in ((INSIDE, False), ((-1.4, 0.2, 4.7), True)):
        d = np.concatenate([S.random_directions(rng, 3000),
                            S.special_directions()])
        rows = S.probe(BOX, origin, d, nmax)
        steps = rows[:, 2].astype(int)
        miss = steps == 0
        assert miss.any() == some_miss
        assert (~miss).sum() > 200
        assert np.isnan(rows[miss, :2]).all() and not rows[miss, 2:].any()
        assert steps.max() <= nmax - 3
        hit = rows[~miss]
        assert (hit[:, 0] >= 0.).all() and (hit[:, 0] < hit[:, 1]).all()
        if not some_miss:
            assert not hit[:, 0].any()
            assert np.allclose(hit[:, 1], S.wall_distance(BOX, origin, d),
                               rtol=1e-14, atol=0.)
        total = hit[:, 3 + nmax:].sum(axis=1)
        scale = np.maximum(np.abs(hit[:, 0]), np.abs(hit[:, 1]))
        assert (np.abs(total - (hit[:, 1] - hit[:, 0])) <= 1e-12 * scale).all()
        cells = hit[:, 3:3 + nmax].astype(np.int64)
        for r in range(len(hit)):
            n = int(hit[r, 2])
            c = cells[r, :n]
            assert (c >= 0).all() and (c < BOX.n).all()
            jump = np.abs(np.diff(unravel(BOX, c), axis=0))
            assert (jump.max(axis=1) == 1).all() if n > 1 else True


PARALLEL_VIEWS = [(0., 0.), (0.7, 0.3), (2.1, 4.0)]


def test_agrees_with_the_plane_parallel_restatement():
    """4: units and orientation. The sky ray from x e_x + y e_y + D n towards
    -n, D beyond the box, crosses the cells of lref's ray through the image
    coordinates (x, y) in reverse order, and both integrate the same cells:
    intensities without and with random extinction agree within 8 eps
    (steps + 1), relative. 8 x 8 pixels in each of three views (one along an
    axis), 192 rays, one per call.

    The two marches reach a cell from opposite sides, so they follow lines
    that differ by the rounding of the positions, delta ~ eps |p| sideways,
    and a path length moves from a cell to its neighbour by that much whatever
    the length of the step. The intensities then differ by delta x (contrast
    between neighbouring cells) per step, which the bound - written for equal
    path lengths - has no room for if the contrast is decades. So: fields
    between 1 and 2 and extinction between 0.2 and 0.6 per unit length (a
    tenth of the cells without dust), which pin units and orientation as
    well as any (no two cells are alike); pixels in the middle 60 % of the
    box's bounding rectangle, so that no chord merely clips an edge; D just
    beyond the box. And 8 pixels across 10 or 12 cells put no pixel centre on
    a cell wall in the axis view (10 i + 5 = 8 k and 6 j + 3 = 4 k have no
    solutions), where the order of the cells would be a matter of ties."""
    rng = np.random.default_rng(4)
    box = BOX
    nf = 3
    fields = rng.uniform(1., 2., (nf, box.n))
    k = rng.uniform(0.2, 0.6, box.n)
    k[rng.uniform(size=box.n) < 0.1] = 0.
    nmax = int(box.ncell.sum()) + 3
    corners = np.array([[box.anchor[a] + ((c >> a) & 1) * box.sides[a]
                         for a in range(3)] for c in range(8)])
    nrays, worst = 0, [0., 0.]
    for theta, phi in PARALLEL_VIEWS:
        n, ex, ey = L.axes(theta, phi)
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        anchor, sides = anchor + 0.2 * sides, 0.6 * sides
        nx = ny = 8
        D = (corners @ n).max() + 0.5
        xy = L.sample_coordinates(nx, ny, anchor, sides)[:, :, 0, 0, :]
        xy = xy.reshape(-1, 2)
        far = L.probe(box, theta, phi, xy, nmax)
        plain = L.render(box, fields, theta, phi, nx, ny, anchor, sides)
        dusty = L.render(box, fields, theta, phi, nx, ny, anchor, sides,
                         extinction=k)
        plain, dusty = plain.reshape(nf, -1), dusty.reshape(nf, -1)
        for p, (x, y) in enumerate(xy):
            origin = x * ex + y * ey + D * n
            row = S.probe(box, origin, -n, nmax)[0]
            steps = int(row[2])
            assert steps == int(far[p, 2]) and steps > 5
            assert np.array_equal(row[3:3 + steps],
                                  far[p, 3:3 + steps][::-1])
            rtol = 8. * EPS * (steps + 1)
            got = S.render(box, fields, origin, -n)[:, 0]
            err = np.abs(got - plain[:, p]) / plain[:, p]
            worst[0] = max(worst[0], err.max() / rtol)
            assert (err <= rtol).all()
            got = S.render(box, fields, origin, -n, extinction=k)[:, 0]
            err = np.abs(got - dusty[:, p]) / dusty[:, p]
            worst[1] = max(worst[1], err.max() / rtol)
            assert (err <= rtol).all()
            nrays += 1
    print("worst difference over its bound: no dust %.3f, dust %.3f" %
          tuple(worst))
    assert nrays == 192


def exact_cell(i, j, k):
    return (i * EXACT.ncell[1] + j) * EXACT.ncell[2] + k


def test_origin_on_a_wall_an_edge_and_a_corner():
    """5, first: the origin exactly on a cell wall, edge and corner of a grid
    whose walls are doubles. The march starts in the cell floor() gives - the
    upper one on every axis that lies on a wall -, and a direction pointing
    back across a wall makes a first step of length 0 that crosses it; every
    axis that ties crosses at once."""
    a, c = EXACT.anchor, EXACT.cellside
    wall_x, wall_y, wall_z = a[0] + 5 * c[0], a[1] + 4 * c[1], a[2] + 9 * c[2]
    mid_y, mid_z = a[1] + 4.3 * c[1], a[2] + 9.6 * c[2]
    s = 1. / np.sqrt(3.)
    unit = lambda v: np.array(v) / np.sqrt(np.dot(v, v))
    cases = [
        # origin, direction, first cell, its ds is 0, second cell
        ((wall_x, mid_y, mid_z), unit([-1., 0.2, 0.1]), (5, 4, 9), True,
         (4, 4, 9)),
        ((wall_x, mid_y, mid_z), unit([1., 0.2, 0.1]), (5, 4, 9), False,
         None),
        ((wall_x, mid_y, mid_z), [-1., 0., 0.], (5, 4, 9), True, (4, 4, 9)),
        ((wall_x, wall_y, mid_z), unit([-1., -1., 0.1]), (5, 4, 9), True,
         (4, 3, 9)),
        ((wall_x, wall_y, mid_z), unit([-1., 1., 0.1]), (5, 4, 9), True,
         (4, 4, 9)),
        ((wall_x, wall_y, mid_z), unit([1., 2., 0.1]), (5, 4, 9), False,
         None),
        ((wall_x, wall_y, wall_z), [-s, -s, -s], (5, 4, 9), True, (4, 3, 8)),
        ((wall_x, wall_y, wall_z), [-s, s, -s], (5, 4, 9), True, (4, 4, 8)),
        ((wall_x, wall_y, wall_z), [s, s, s], (5, 4, 9), False, (5, 5, 9)),
    ]
    for origin, d, first, zero, second in cases:
        row = S.probe(EXACT, origin, d, 40)[0]
        steps = int(row[2])
        assert steps >= 2 and row[0] == 0. and row[1] > 0.
        assert row[3] == exact_cell(*first), (origin, d)
        assert (row[3 + 40] == 0.) == zero, (origin, d)
        assert (row[3 + 40:3 + 40 + steps] >= 0.).all()
        if second is not None:
            assert row[4] == exact_cell(*second), (origin, d)
        if zero:
            assert row[4 + 40] > 0.
        # the zero-length step adds nothing to an intensity
        chord = S.wall_distance(EXACT, origin, d)[0]
        got = S.render(EXACT, np.full(EXACT.n, 2.), origin, d,
                       extinction=np.full(EXACT.n, 0.4))[0, 0]
        want = 2. / (FOURPI * 0.4) * -np.expm1(-0.4 * chord)
        assert np.isclose(got, want, rtol=1e-12, atol=0.)


def test_origin_on_a_box_face_and_outside():
    """5, the rest: from a box face outwards there is nothing (a miss),
    inwards the whole chord; an origin on the upper face starts in the last
    cell; rays from outside that miss give 0"""
    a, s = EXACT.anchor, EXACT.sides
    mid = a + 0.43 * s
    for axis in range(3):
        for side, sign in ((0., -1.), (1., 1.)):
            origin = mid.copy()
            origin[axis] = a[axis] + side * s[axis]
            d = np.zeros(3)
            d[axis] = sign
            out = S.probe(EXACT, origin, d, 20)[0]
            assert out[2] == 0. and np.isnan(out[:2]).all()
            tilted = d + 0.3
            tilted[axis] = sign
            tilted /= np.sqrt(np.dot(tilted, tilted))
            assert S.probe(EXACT, origin, tilted, 20)[0, 2] == 0.
            assert S.render(EXACT, np.ones(EXACT.n), origin, tilted)[0, 0] == 0.
            back = S.probe(EXACT, origin, -d, 20)[0]
            assert back[2] == EXACT.ncell[axis]
            assert back[0] == 0. and back[1] == s[axis]
            first = unravel(EXACT, np.array([int(back[3])]))[0]
            assert first[axis] == (0 if side == 0. else EXACT.ncell[axis] - 1)
            assert np.isclose(back[3 + 20:].sum(), s[axis], rtol=1e-14)
    # outside: towards the box some rays hit, away from it none does
    origin = a - np.array([2., 1., 3.])
    d = S.random_directions(np.random.default_rng(6), 4000)
    rows = S.probe(EXACT, origin, d, 0)
    img = S.render(EXACT, np.ones(EXACT.n), origin, d)[0]
    hit = rows[:, 2] > 0
    assert 50 < hit.sum() < 2000
    assert (img[hit] > 0.).all() and not img[~hit].any()
    assert (rows[hit, 0] > 0.).all()
    assert not hit[(d < 0.).all(axis=1)].any()


def test_sky_map_directions():
    """6: unit vectors at the pixel centres, pixel (i, j) at i * nlat + j;
    the solid angles add up to 4 pi for the full sky and to the window's
    area otherwise"""
    from cmacionize_amd import engine as E
    nlon, nlat = 37, 19
    d, omega = E.sky_map_directions(nlon, nlat)
    assert d.shape == (nlon * nlat, 3) and omega.shape == (nlon * nlat,)
    assert np.abs((d * d).sum(axis=1) - 1.).max() < 1e-15
    assert np.isclose(omega.sum(), FOURPI, rtol=1e-14, atol=0.)
    assert (omega > 0.).all()
    i, j = 11, 5
    lon = -np.pi + 2. * np.pi * (i + 0.5) / nlon
    lat = -HALF + np.pi * (j + 0.5) / nlat
    want = [np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)]
    assert np.allclose(d[i * nlat + j], want, rtol=0., atol=1e-15)
    # a window in a turned frame
    c, s = np.cos(0.4), np.sin(0.4)
    frame = np.array([[c, s, 0.], [0., 0., 1.], [s, -c, 0.]])
    lon_range, lat_range = (0.2, 1.7), (-0.3, 0.9)
    d, omega = E.sky_map_directions(8, 5, lon_range, lat_range, frame)
    area = (lon_range[1] - lon_range[0]) * \
        (np.sin(lat_range[1]) - np.sin(lat_range[0]))
    assert np.isclose(omega.sum(), area, rtol=1e-14, atol=0.)
    lon = lon_range[0] + 1.5 * (3 + 0.5) / 8
    lat = lat_range[0] + 1.2 * (4 + 0.5) / 5
    want = np.cos(lat) * np.cos(lon) * frame[0] + \
        np.cos(lat) * np.sin(lon) * frame[1] + np.sin(lat) * frame[2]
    assert np.allclose(d[3 * 5 + 4], want, rtol=0., atol=1e-15)
    assert np.abs((d * d).sum(axis=1) - 1.).max() < 1e-15
    # what the host refuses
    for bad in (dict(nlon=0), dict(nlat=-1), dict(lon_range=(1., 1.)),
                dict(lat_range=(-2., 1.)), dict(lat_range=(0.5, 0.2)),
                dict(frame=[[1., 0., 0.], [0., 1., 0.], [0., 1e-6, 1.]]),
                dict(frame=2. * np.eye(3)),
                dict(lon_range=(0., np.inf))):
        args = dict(nlon=4, nlat=4)
        args.update(bad)
        with pytest.raises(E.EngineError):
            E.sky_map_directions(**args)


def test_library_exports_the_sky_symbols():
    """7, first"""
    from cmacionize_amd import engine
    names = ["cmi_gpu_render_line_sky", "cmi_gpu_render_field_sky",
             "cmi_gpu_sky_probe", "cmi_gpu_render_line_sky_map"]
    lib = C.CDLL(engine.LIB_PATH)
    for name in names:
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    for name in ("render_line_sky", "render_field_sky", "sky_probe",
                 "render_line_sky_map"):
        assert callable(getattr(engine.GpuEngine, name))
    assert callable(engine.sky_map_directions)


OBSERVER = "  observer position: [0. m, 0. m, 0. m]\n"


@pytest.mark.parametrize("block,message", [
    ("  number of longitude pixels: 90\n", "observer position is required"),
    (OBSERVER + "  type: JPEG\n", "EmissionSkyMaps:type"),
    (OBSERVER + "  number of longitude pixels: 0\n", "longitude pixels"),
    (OBSERVER + "  number of latitude pixels: -4\n", "latitude pixels"),
    (OBSERVER + "  longitude range: [10. degrees, 10. degrees]\n",
     "longitude range"),
    (OBSERVER + "  latitude range: [-100. degrees, 90. degrees]\n",
     "latitude range"),
    (OBSERVER + "  latitude range: 30. degrees\n", "latitude range"),
    (OBSERVER + "  dust cross section per hydrogen: -1. m^2\n",
     "cross section"),
    (OBSERVER + "  frame pole: [0., 0., 2.]\n"
     "  frame zero longitude: [0., 0., -1.]\n", "parallel"),
    (OBSERVER + "  frame pole: [0., 0., 0.]\n", "not zero"),
])
def test_driver_refuses_a_bad_block_first(tmp_path, block, message):
    """7, second: a bad EmissionSkyMaps block ends `cmi-gpu --emission` with
    its message before the snapshot is opened or a device touched: the
    snapshot named here does not exist, and that is not what the run
    complains of"""
    params = tmp_path / "lines.param"
    params.write_text("EmissivityValues:\n  Halpha: true\n"
                      "EmissionSkyMaps:\n" + block)
    r = subprocess.run([CMI_GPU, "--emission", "--params", str(params),
                        "--file", str(tmp_path / "nowhere.hdf5")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(str(params) + ".used-values")


def test_driver_reads_the_block_only_if_it_is_there(tmp_path):
    """7, third: a good block is read whole, defaults included, before the
    snapshot is looked for; without the block the used-values do not mention
    any of its keys"""
    exits = {}
    for name, block in (("with", "EmissionSkyMaps:\n" + OBSERVER +
                         "  frame pole: [0., 1., 1.]\n"), ("without", "")):
        params = tmp_path / (name + ".param")
        params.write_text("EmissivityValues:\n  Halpha: true\n" + block)
        r = subprocess.run([CMI_GPU, "--emission", "--params", str(params),
                            "--file", str(tmp_path / "nowhere.hdf5")],
                           capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode != 0 and "Could not open" in r.stderr
        exits[name] = open(str(params) + ".used-values").read()
    used = exits["with"]
    for key in ("EmissionSkyMaps:", "observer position", "frame pole",
                "number of longitude pixels: 360",
                "number of latitude pixels: 180", "longitude range",
                "latitude range", "frame zero longitude", "type: BinaryArray",
                "filename prefix: sky_map", "output folder"):
        assert key in used, key
    used = exits["without"]
    assert "Halpha: true" in used
    for key in ("EmissionSkyMaps", "observer", "pixels", "range", "frame",
                "sky_map"):
        assert key not in used, key
