"""The probes of one camera report one and the same walk (csrc/ray_walk.h):
line_image_probe, continuum_probe and absorbing_cube_probe for the parallel
camera, sky_probe, continuum_probe and absorbing_cube_probe for the rays from
a point. The columns {t0, t1, steps, cells, ds} of the three must be equal
bit for bit, misses, axis-parallel rays, rays on cell walls and on the box's
faces included. The grid has unequal cell counts (a transposed index shows)
and sides whose cell walls are exact binary numbers (a ray can lie exactly on
one)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCELL = (3, 4, 5)
ANCHOR = (-1.5, -1., 0.5)
SIDES = (3., 2., 2.5)          # cells of 1 x 0.5 x 0.5
MAX_CELLS = 16                 # the longest walk crosses 3 + 4 + 5 - 2 = 10
NCHAN, VMIN, VMAX = 2, -4., 4.
PREFIX = 3 + 2 * MAX_CELLS


@pytest.fixture(scope="module")
def eng():
    from cmacionize_amd import GpuEngine
    engine = GpuEngine(NCELL, ANCHOR, SIDES, (0, 0, 0), device=0)
    yield engine
    engine.close()


@pytest.fixture(scope="module")
def cells():
    """random positive fields, shared and left unchanged"""
    rng = np.random.default_rng(17)
    n = int(np.prod(NCELL))
    f = dict(kappa=10. ** rng.uniform(-1., 0.5, (NCHAN, n)),
             source=rng.uniform(0.5, 2., (NCHAN, n)),
             a=10. ** rng.uniform(-1., 0.5, n),
             sl=rng.uniform(0.5, 2., n),
             b=rng.uniform(1., 3., n))
    for x in f.values():
        x.setflags(write=False)
    return f


def generic_view_rays():
    """a view along no axis: a 4 x 4 lattice of image coordinates around the
    box's centre (its projection is the image's origin shifted by the
    centre's), and four rays that miss"""
    theta, phi = 0.7, 0.3
    st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    centre = np.array(ANCHOR) + 0.5 * np.array(SIDES)
    cx = centre @ np.array([-sp, cp, 0.])
    cy = centre @ np.array([-ct * cp, -ct * sp, st])
    t = np.array([-0.7, -0.2, 0.3, 0.8])
    hits = [(cx + u, cy + w) for u in t for w in t]
    misses = [(cx + 9., cy), (cx, cy - 9.), (cx - 9., cy + 9.), (1.e6, 1.e6)]
    return theta, phi, np.array(hits + misses)


def axis_view_rays():
    """theta = phi = 0: n = (0, 0, 1) exactly, e_x = (0, 1, 0), e_y = (-1, 0,
    0), so that image coordinates (x, y) are the line (-y, x, .) along z"""
    def at(px, py):
        return (py, -px)
    rays = [
        at(-1.25, -0.875), at(0.25, 0.125), at(1.125, 0.75),   # generic
        at(-0.5, 0.125), at(0.5, -0.75),     # on a wall across x
        at(0.25, 0.), at(-1.25, -0.5),       # on a wall across y
        at(-0.5, 0.), at(0.5, 0.5), at(-0.5, -0.5),   # on a cell edge
        at(-1.5, 0.125), at(0.25, -1.), at(-1.5, -1.),   # the lower faces
        at(1.5, 0.125), at(0.25, 1.), at(1.5, 1.),    # the upper faces: miss
        at(-1.75, 0.), at(0., 1.25), at(40., 40.),    # outside
    ]
    return 0., 0., np.array(rays)


def check_rows(rows, what):
    """the three probes' prefixes are equal; at least half of the rays hit
    and take three steps or more"""
    first = rows[0][:, :PREFIX]
    for other in rows[1:]:
        assert np.array_equal(first, other[:, :PREFIX], equal_nan=True), what
    steps = first[:, 2]
    assert 2 * np.count_nonzero(steps >= 3) >= len(steps), (what, steps)
    assert np.count_nonzero(steps == 0) >= 3, (what, steps)
    assert np.isnan(first[steps == 0, :2]).all(), what
    assert steps.max() <= MAX_CELLS
    return first


@pytest.mark.parametrize("rays", [generic_view_rays, axis_view_rays])
def test_parallel_camera_probes_walk_alike(eng, cells, rays):
    theta, phi, xy = rays()
    rows = [
        eng.line_image_probe(theta, phi, xy, MAX_CELLS),
        eng.continuum_probe(cells["kappa"], cells["source"], xy, MAX_CELLS,
                            theta=theta, phi=phi),
        eng.absorbing_cube_probe(cells["a"], cells["sl"], cells["b"], xy,
                                 MAX_CELLS, NCHAN, VMIN, VMAX, theta=theta,
                                 phi=phi),
    ]
    first = check_rows(rows, rays.__name__)
    if rays is axis_view_rays:
        # a line along z crosses the five cells of its column, 0.5 each
        hit = first[:, 2] > 0
        assert np.count_nonzero(hit) == 13
        assert np.all(first[hit, 2] == NCELL[2])
        assert np.all(first[hit, 3 + MAX_CELLS:3 + MAX_CELLS + 5] == 0.5)
        # the ray on both lower faces walks column 0, 0 towards the observer
        assert np.array_equal(first[12, 3:8], np.arange(NCELL[2]))


def point_camera_rays():
    """(origin, directions) pairs: the origins in the box see all directions,
    those on its upper face x = 1.5 and outside it the same lines turned
    towards -x, and two that point away"""
    s = np.sqrt(0.5)
    d = np.array([
        (0.6, 0.48, 0.64), (-0.36, 0.8, -0.48), (0.48, -0.6, 0.64),
        (-0.8, -0.36, -0.48),                               # generic
        (1., 0., 0.), (-1., 0., 0.), (0., 1., 0.), (0., -1., 0.),
        (0., 0., 1.), (0., 0., -1.),                        # along an axis
        (s, s, 0.), (-s, 0., s), (0., s, -s), (0.6, 0.8, 0.),   # in a face
    ] + [np.array(q) / 7. for q in (
        (2., 3., 6.), (-6., 2., 3.), (3., -6., -2.), (-2., -6., 3.),
        (6., -3., 2.), (-3., 2., -6.))])                    # generic
    origins = [
        (-1.2, -0.8, 0.7),      # inside, on no wall
        (-0.5, 0.2, 1.7),       # on the inner wall x = -0.5
        (-0.5, 0., 1.5),        # on a cell corner
        (1.5, 0.2, 1.7),        # on the box's upper face
        (1.75, 0.3, 1.8),       # outside
    ]
    inward = np.concatenate([np.where(d[:, :1] > 0., -d, d),
                             [(1., 0., 0.), (0.6, 0.8, 0.)]])
    return [(np.array(o), d if i < 3 else inward)
            for i, o in enumerate(origins)]


def test_point_camera_probes_walk_alike(eng, cells):
    prefix = []
    for origin, d in point_camera_rays():
        assert np.all(np.abs((d * d).sum(axis=1) - 1.) <= 1.e-9)
        rows = [
            eng.sky_probe(origin, d, MAX_CELLS),
            eng.continuum_probe(cells["kappa"], cells["source"], d, MAX_CELLS,
                                origin=origin),
            eng.absorbing_cube_probe(cells["a"], cells["sl"], cells["b"], d,
                                     MAX_CELLS, NCHAN, VMIN, VMAX,
                                     origin=origin),
        ]
        for other in rows[1:]:
            assert np.array_equal(rows[0][:, :PREFIX], other[:, :PREFIX],
                                  equal_nan=True), origin
        prefix.append(rows[0][:, :PREFIX])
    steps = np.concatenate([p[:, 2] for p in prefix])
    assert 2 * np.count_nonzero(steps >= 3) >= len(steps), steps
    assert np.count_nonzero(steps == 0) >= 3, steps
    assert steps.max() <= MAX_CELLS
    # the origin on the wall x = -0.5: towards -x the walk starts in the cell
    # above the wall with a step of length 0, towards +x with a whole cell
    wall = prefix[1]
    assert wall[5, 3 + MAX_CELLS] == 0. and wall[4, 3 + MAX_CELLS] == 1.
    assert wall[5, 2] == 2 and wall[4, 2] == 2
    # from outside, only the rays towards the box arrive: t0 > 0
    outside = prefix[4]
    assert outside[5, 0] == 0.25 and np.isnan(outside[-2, 0])
