"""GPU tests of the scattered-light sky maps: the point camera of the dust
kernels (cmi_gpu_set_sky_camera, dust_shoot_kernel / dust_probe_kernel for
the cell source and DUST_CAMERA_POINT), GpuEngine.render_scattered_line_sky_map
and `cmi-gpu --emission` with `EmissionSkyMaps:scattering: true` - against the
CPU restatement tests/support/scattered_sky_reference.c on the same random
streams (checked on its own in test_scattered_sky_host.py).

Tolerances are those test_gpu_dust.py derives in its module docstring, one
per quantity:
  r (a subtraction, three products, a square root: no transcendental) - its
    positions' 1e-13 of the box side, relative here;
  tau to the observer - its optical depths have no transcendental and are
    equal there; here the march's direction k = v / r is as exact, so the
    sums are compared at rtol 1e-13 and the steps must be equal;
  hgfac - test_scatter_towards' rtol 1e-13;
  Stokes after the peel-off - test_scatter_towards' 1e-12 of I; the rotation
    to the frame's pole divides by the lengths of two projections, which
    amplifies by 1 / |N| (|N| = the sine of the angle between k and the
    pole), so rows with |N| < 1e-2 for either pole are compared at 1e-10;
  traces - test_traces' 1e-12 of the side for positions, 1e-11 of I for
    Stokes, rtol 1e-11 for the weight (here W / r^2);
  whole runs - test_whole_run's rtol 1e-9 per pixel;
  additivity - test_additive's rtol 1e-12, atol 1e-14 of the largest I."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scattered_line_lib as SL
import scattered_sky_lib as K
import test_gpu_dust as D
from test_gpu_dust import SEED, _bad_pixels, _culprits, _on_box_face

pytestmark = pytest.mark.gpu

ALBEDO = 0.6
OBSERVER = np.array(K.IDENTITY_OBSERVER)
TILTED = K.frame_of((0.2, -0.4, 0.8), (1., 0.3, 0.))
CAMERAS = {
    # inside, Q and U rotated to a tilted pole
    "inside": K.Camera(OBSERVER, 24, 12, 0.05, frame=TILTED),
    # the pole exactly z: the unrotated path; a window with the seam in it
    "window": K.Camera(OBSERVER, 9, 7, 0.05, lon=(2.5, 2.5 + 1.5 * np.pi),
                       lat=(-1.2, 0.9)),
    # outside the box: the march leaves the grid before it reaches r
    "outside": K.Camera((2.6, 1.1, 5.3), 24, 12, 0., frame=TILTED),
}


@pytest.fixture(scope="module")
def scene():
    """the 10 x 12 x 9 grid of the statistical identity with albedo 0.6:
    engine (cell source set) and what a restatement needs"""
    box, model, field = SL.identity_model(ALBEDO)
    eng = SL.make_engine(model, field)
    yield model, field, eng
    eng.close()


def _pixel_coordinates(cam, x):
    """fractional pixel coordinates of the positions x, and r"""
    l, b, r = cam.angles(x)
    u = np.mod(l - cam.lon[0], 2. * np.pi) / (cam.lon[1] - cam.lon[0]) * \
        cam.nlon
    v = (b - cam.lat[0]) / (cam.lat[1] - cam.lat[0]) * cam.nlat
    return u, v, r


def _is_edge_case(cam, x, tol=1e-9):
    """a direction within rounding of a pixel edge (the seam and the window's
    edges are pixel edges), or r within rounding of the exclusion radius"""
    u, v, r = _pixel_coordinates(cam, np.asarray(x))
    near = min(abs(u - round(u)), abs(v - round(v))) < tol
    return bool(near or abs(r - cam.r_min) <= tol * max(cam.r_min, 1e-300))


# ------------------------------------------------------------- SKY_PEEL --

def _peel_rows(model, cam, n):
    """random (position, direction, Stokes) rows and the special ones"""
    rng = np.random.default_rng(17)
    rows = np.zeros((n, 15))
    rows[:, 0:3] = model.anchor + rng.uniform(size=(n, 3)) * model.sides
    rows[:, 3:15] = D._rows(n, 6, True)
    (e1, e2, e3) = cam.frame
    cell = model.sides / model.ncell
    r_min = max(cam.r_min, 0.05)
    centre = model.anchor + 0.5 * model.sides
    lo, hi = model.anchor, model.anchor + model.sides
    if not (np.all(cam.origin >= lo) and np.all(cam.origin <= hi)):
        # an observer outside the box: photons are in the box, so the special
        # directions are laid through its centre c - straight below the
        # observer is not in the box; rows on the line from c towards the
        # observer, c's cell, and points whose sky direction is on the seam
        # (p - o along -e_1 is not in the box either: the rows in the plane
        # of e_1 and e_3 through c that look nearest to it) are what is left
        to = cam.origin - centre
        to /= np.sqrt(to @ to)
        special = [centre, centre + 0.4 * to, centre - 0.6 * to,
                   centre + 0.3 * cell * [1., -1., 0.5],
                   centre + [0.5, -0.3, cam.origin[2] - centre[2] - 2.3],
                   centre + 0.9 * to + 1e-13 * e2,
                   centre + 0.3 * e3, centre - 0.3 * e3,
                   centre + 0.4 * e1, centre - 0.4 * e1]
        for x in special:
            assert np.all(x >= lo) and np.all(x < hi), x
        rows[2:2 + len(special), 0:3] = np.array(special)
        return rows, 2 + len(special)
    o = cam.origin
    special = [
        o - [0., 0., 0.4], o + [0., 0., 0.3],        # sin theta == 0
        o + [0.5, -0.3, 0.], o + [-0.2, 0., 0.],     # k in the xy plane
        o + 0.3 * cell * [1., -1., 0.5],             # the observer's own cell
        o + 0.06 * e2,
        o + r_min * (1. - 1e-9) * e2, o + r_min * (1. + 1e-9) * e2,
        o + r_min * (1. - 1e-9) * np.array([0.6, 0., 0.8]),
        o + r_min * (1. + 1e-9) * np.array([0.6, 0., 0.8]),
        o - 0.4 * e1, o - 0.4 * e1 + 1e-13 * e2,     # the longitude seam
        o - 0.4 * e1 - 1e-13 * e2, o - 0.7 * e1 + 1e-4 * e2,
        o + 0.5 * e3, o - 0.5 * e3,                  # the polar rows
        o + 0.5 * e3 + 1e-3 * e1, o - 0.5 * e3 - 1e-3 * e2,
    ]
    rows[2:2 + len(special), 0:3] = np.array(special)
    return rows, 2 + len(special)


def test_probe_rows_past_one_launch(scene):
    """The point camera's probe instantiation with more rows than one launch
    of cmi_gpu_dust_probe takes (2^14): the rows past it are the rows probed
    alone, with first_packet moved up by 2^14."""
    from cmacionize_amd import engine as E
    import test_gpu_dust as D
    model, field, eng = scene
    CAMERAS["inside"].apply(eng)
    launch = 1 << 14
    rows = D._rows(launch + 50, 5, True)
    gpu = eng.dust_probe(E.DUST_PROBE_SCATTER, SEED, 7, len(rows), rows)
    alone = eng.dust_probe(E.DUST_PROBE_SCATTER, SEED, 7 + launch, 50,
                           rows[launch:])
    assert np.abs(gpu[launch:, 8]).min() > 0.
    assert np.array_equal(gpu[launch:], alone)


@pytest.mark.parametrize("name", list(CAMERAS))
def test_sky_peel_rows(scene, name):
    """7. One peel-off per row against the restatement."""
    from cmacionize_amd import engine as E
    model, field, eng = scene
    cam = CAMERAS[name]
    cam.apply(eng)
    ref = K.Restatement(model, field, cam)
    rows, nspecial = _peel_rows(model, cam, 4000)
    gpu = eng.dust_probe(E.DUST_PROBE_SKY_PEEL, 0, 0, len(rows), rows)
    cpu = ref.peel(rows)
    # the special rows do what they are there for
    pix = cpu[:, 8]
    assert (pix >= 0).sum() > 1000
    if name != "outside":
        assert (pix[:nspecial] == -2).sum() >= 2
        assert cpu[pix != -2, 7].min() == 1.  # clipped in the first step
    else:
        assert not (pix == -2).any()
    if name == "window":
        assert (pix == -1).sum() > 100
    differ = np.flatnonzero(gpu[:, 8] != cpu[:, 8])
    print(name, "rows whose pixel differs:", list(differ))
    for k in differ:
        assert _is_edge_case(cam, rows[k, :3]), (k, gpu[k], cpu[k])
    same = gpu[:, 8] == cpu[:, 8]
    seen = same & (cpu[:, 8] != -2)
    assert np.array_equal(gpu[same, 7], cpu[same, 7])       # steps
    assert np.allclose(gpu[same, 5], cpu[same, 5], rtol=1e-13, atol=0.)   # r
    assert np.allclose(gpu[seen, 6], cpu[seen, 6], rtol=1e-13, atol=0.)   # tau
    assert np.allclose(gpu[seen, 0], cpu[seen, 0], rtol=1e-13, atol=0.)
    assert cpu[seen, 6].max() > 0.5
    # Stokes: 1e-12 of I, 1e-10 where a pole lies within 1e-2 of k
    v = cam.origin - rows[:, :3]
    k = v / np.sqrt((v * v).sum(axis=1))[:, None]
    sine = np.minimum(np.sqrt(np.maximum(1. - k[:, 2] ** 2, 0.)),
                      np.sqrt(np.maximum(1. - (k @ cam.frame[2]) ** 2, 0.)))
    near_pole = sine < 1e-2
    # the looser bound is confined to the special rows laid along a pole and
    # the odd random row (two poles' four caps of 1e-2 rad are 1e-4 of the
    # sphere: 0.4 rows of 4000 expected)
    print(name, "rows within 1e-2 of a pole:", list(np.flatnonzero(near_pole)))
    assert near_pole[nspecial:].sum() <= 3
    if name != "outside":
        assert 2 <= near_pole[:nspecial].sum() <= 8
    tol = np.where(near_pole, 1e-10, 1e-12)[:, None]
    I = np.abs(cpu[:, 1:2])
    err = np.abs(gpu[:, 1:5] - cpu[:, 1:5])
    assert np.all(err[seen] <= (tol * I)[seen]), \
        np.max((err / np.maximum(tol * I, 1e-300))[seen])
    # excluded rows: r and the code, nothing else
    gone = same & (cpu[:, 8] == -2)
    assert not gpu[gone][:, [0, 1, 2, 3, 4, 6, 7]].any()


# --------------------------------------------------------------- traces --

def test_traces(scene):
    """8. test_gpu_scattered_line.py::test_traces with the point camera, and
    the same packets as the parallel camera on the device."""
    from cmacionize_amd import engine as E
    model, field, eng = scene
    # (an exclusion radius of a cell side: some of the 2000 packets' events
    # fall inside it)
    cam = K.Camera(OBSERVER, 24, 12, 0.25, frame=TILTED)
    ref = K.Restatement(model, field, cam)
    d = model.describe()
    n, cap = 2000, 64
    eng.set_ccd_image(model.theta, model.phi, model.nx, model.ny,
                      model.img_anchor, model.img_sides)
    parallel = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, n, None, cap)
    cam.apply(eng)
    gpu = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, n, None, cap)
    cpu = ref.trace(SEED, 0, n, cap)
    # no random number: event for event the parallel camera's positions
    assert np.array_equal(gpu[:, [0, 1, 3]], parallel[:, [0, 1, 3]])
    assert np.array_equal(gpu[:, 4:].reshape(n, cap, 8)[:, :, :3],
                          parallel[:, 4:].reshape(n, cap, 8)[:, :, :3])
    assert np.all(gpu[:, 3] == 0.)
    assert cpu[:, 1].max() >= 2 and cpu[:, 0].max() < cap
    side = model.sides.max()
    ev = np.minimum(np.minimum(cpu[:, 0], gpu[:, 0]), cap).astype(int)
    g = gpu[:, 4:].reshape(n, cap, 8)
    c = cpu[:, 4:].reshape(n, cap, 8)
    for k in np.flatnonzero(gpu[:, 0] != cpu[:, 0]):
        longer = g[k] if gpu[k, 0] > cpu[k, 0] else c[k]
        assert ev[k] < cap
        assert _on_box_face(d, longer[ev[k], 0:3]), (k, gpu[k, :4], cpu[k, :4])
    excluded = 0
    for k in range(n):
        a, b = g[k, :ev[k]], c[k, :ev[k]]
        assert np.allclose(a[:, 0:3], b[:, 0:3], rtol=0., atol=1e-12 * side), k
        flip = (a[:, 7] == 0.) != (b[:, 7] == 0.)
        for x in b[flip, 0:3]:  # r within rounding of the exclusion radius
            assert _is_edge_case(cam, x), (k, x)
        a, b = a[~flip], b[~flip]
        excluded += int((b[:, 7] == 0.).sum())
        assert np.allclose(a[:, 3:7], b[:, 3:7], rtol=0.,
                           atol=1e-11 * np.abs(b[:, 3:4])), k
        assert np.allclose(a[:, 7], b[:, 7], rtol=1e-11, atol=0.), k
    assert excluded > 0


def test_a_packet_alone_is_the_packet_among_others(scene):
    """9, first: the guard of DESIGN.md 4.6 for the new instantiation."""
    from cmacionize_amd import engine as E
    model, field, eng = scene
    CAMERAS["inside"].apply(eng)
    cap = 64
    among = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, 0, 64, None, cap)
    assert among[:, 1].max() >= 2
    for k in (0, 1, 17, 31, 32, 63, int(np.argmax(among[:, 1]))):
        alone = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, k, 1, None, cap)[0]
        assert np.array_equal(alone, among[k]), k


def test_additive(scene):
    """9, second"""
    model, field, eng = scene
    CAMERAS["inside"].apply(eng)
    N, a = 30000, 12345
    eng.dust_shoot(SEED, 0, N)
    whole = eng.download_image()
    counters = eng.get_sky_camera_counters()
    eng.reset_image()
    eng.dust_shoot(SEED, 0, a)
    eng.dust_shoot(SEED, a, N - a)
    parts = eng.download_image()
    c = eng.get_dust_counters()
    assert c["ncapped"] == 0 and c["npackets"] == N
    assert eng.get_sky_camera_counters() == counters
    atol = 1e-14 * np.abs(whole[0]).max()
    assert np.allclose(parts, whole, rtol=1e-12, atol=atol)


# ------------------------------------------------------------ whole run --

class _NoPixels:
    """for test_gpu_dust._is_threshold_case: skips its pixel comparison (the
    parallel camera's) and leaves its comparison of the numbers of events"""

    @staticmethod
    def pixel(x):
        return 0


def _is_threshold_case(d, cam, ref, gpu_tr, cpu_tr, cap):
    """the trace of a culprit: the first event whose pixel (or exclusion)
    differs between the two sides is an edge case; or the number of events
    differs as test_gpu_dust._is_threshold_case accepts"""
    g = gpu_tr[4:].reshape(cap, 8)
    c = cpu_tr[4:].reshape(cap, 8)
    n = int(min(gpu_tr[0], cpu_tr[0], cap))
    for k in range(n):
        if ref.pixel(g[k, :3]) != ref.pixel(c[k, :3]):
            return _is_edge_case(cam, c[k, :3])
    return D._is_threshold_case(d, _NoPixels, gpu_tr, cpu_tr, cap)


@pytest.mark.parametrize("name", ["inside", "window"])
def test_whole_run(scene, name):
    """10. test_gpu_dust.py::test_whole_run_32's scheme: rtol 1e-9 per
    pixel; packets behind a differing pixel are bisected and shown to be
    threshold cases; equal counters - the camera's two among them - when no
    pixel differs"""
    from cmacionize_amd import engine as E
    model, field, eng = scene
    cam = CAMERAS[name] if name == "window" else \
        K.Camera(OBSERVER, 24, 12, 0.25, frame=TILTED)
    cam.apply(eng)
    ref = K.Restatement(model, field, cam)
    d = model.describe()
    N = 50000
    eng.dust_shoot(SEED, 0, N)
    gpu = eng.download_image()
    c = eng.get_dust_counters()
    s = eng.get_sky_camera_counters()
    cpu, cc = ref.shoot(SEED, 0, N)
    assert gpu.shape == cpu.shape == (3, cam.nlon, cam.nlat)
    assert c["npackets"] == N and c["ncapped"] == 0 and cc[2] == 0
    assert c["nsource_capped"] == 0
    assert np.count_nonzero(cpu[0]) > 50 and cc[1] > N
    assert np.abs(cpu[1]).max() > 0. and np.abs(cpu[2]).max() > 0.
    if name == "inside":
        assert cc[4] > 0
    else:
        assert cc[5] > 0
    bad = _bad_pixels(gpu, cpu)
    print("differing pixels", int(bad.sum()))
    if not np.any(bad):
        assert c["nscatter"] == cc[1]
        assert c["nsteps"] == cc[0]
        assert s == {"nexcluded": cc[4], "noutside": cc[5]}
        return
    culprits = []
    _culprits(eng, ref, 0, N, bad, culprits)
    assert culprits, "differing pixels without a differing packet"
    cap = 4096
    for k in culprits:
        gt = eng.dust_probe(E.DUST_PROBE_TRACE, SEED, k, 1, None, cap)[0]
        ct = ref.trace(SEED, k, 1, cap)[0]
        assert _is_threshold_case(d, cam, ref, gt, ct, cap), k
    ok = np.ones(N, bool)
    ok[culprits] = False
    gpu2 = np.zeros_like(gpu)
    cpu2 = np.zeros_like(cpu)
    edges = np.flatnonzero(np.diff(np.r_[0, ok.astype(int), 0]))
    for lo, hi in zip(edges[0::2], edges[1::2]):
        eng.reset_image()
        eng.dust_shoot(SEED, int(lo), int(hi - lo))
        gpu2 += eng.download_image()
        cpu2 += ref.shoot(SEED, int(lo), int(hi - lo))[0]
    assert not np.any(_bad_pixels(gpu2, cpu2))


# ----------------------------------------------- switching and refusals --

def test_camera_switching_and_refusals():
    """13."""
    from cmacionize_amd import engine as E
    lib = E.load_library()
    box, model, field = SL.identity_model(ALBEDO)
    cam = CAMERAS["inside"]
    N = 5000

    fresh = SL.make_engine(model, field)
    fresh.dust_shoot(SEED, 0, N)
    want = fresh.download_image()
    fresh.close()

    from cmacionize_amd import GpuEngine
    eng = GpuEngine(tuple(int(v) for v in model.ncell), tuple(model.anchor),
                    tuple(model.sides), (0, 0, 0), device=0)
    eng.upload_cells(model.density, np.zeros(model.n), None)
    eng.set_dust_scattering_per_hydrogen(model.g, model.p_l, model.albedo,
                                         model.sigma)
    eng.set_cell_source_field(field)
    # no camera yet
    assert lib.cmi_gpu_dust_shoot(eng._h, SEED, 0, 10) == K.ESTATE
    assert lib.cmi_gpu_download_image(eng._h, None, None, None) == K.ESTATE

    def works():
        cam.apply(eng)
        eng.dust_shoot(SEED, 0, N)
        image = eng.download_image()
        assert image.shape == (3, cam.nlon, cam.nlat) and image[0].sum() > 0.
        return image

    first = works()
    # SKY_PEEL needs the point camera
    eng.set_ccd_image(model.theta, model.phi, model.nx, model.ny,
                      model.img_anchor, model.img_sides)
    out = np.zeros(9)
    assert lib.cmi_gpu_dust_probe(eng._h, E.DUST_PROBE_SKY_PEEL, SEED, 0, 1,
                                  SL._p(np.ones(15)), SL._p(out), 0) == \
        K.ESTATE
    assert b"sky camera" in lib.cmi_gpu_last_error()
    # ... and the parallel image is a fresh engine's
    eng.dust_shoot(SEED, 0, N)
    back = eng.download_image()
    assert back.shape == want.shape
    assert np.allclose(back, want, rtol=1e-12,
                       atol=1e-14 * np.abs(want[0]).max())
    assert eng.get_sky_camera_counters() == {"nexcluded": 0, "noutside": 0}
    again = works()
    assert np.allclose(again, first, rtol=1e-12,
                       atol=1e-14 * np.abs(first[0]).max())
    # a refused camera leaves the one that is set
    f = SL._f64(cam.frame).reshape(9)
    o = SL._f64(cam.origin)
    assert lib.cmi_gpu_set_sky_camera(
        eng._h, SL._p(o), SL._p(f), -np.pi, np.pi, -0.5 * np.pi, 0.5 * np.pi,
        8, 4, 0., 1) == K.EINVAL
    assert b"exclusion radius" in lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_set_sky_camera(
        eng._h, SL._p(o), SL._p(f), -np.pi, 3.5 * np.pi, -0.5 * np.pi,
        0.5 * np.pi, 8, 4, 0.1, 1) == K.EINVAL
    eng.reset_image()
    eng.dust_shoot(SEED, 0, N)
    assert np.allclose(eng.download_image(), first, rtol=1e-12,
                       atol=1e-14 * np.abs(first[0]).max())
    eng.close()

    # the galaxy source has no point camera (a box around the origin)
    g = GpuEngine((8, 8, 8), (-1., -1., -1.), (2., 2., 2.), (0, 0, 0),
                  device=0)
    g.upload_cells(np.ones(512), np.zeros(512), None)
    g.set_dust_scattering_per_hydrogen(0.4, 0.3, 0.5, 0.3)
    g.set_continuous_source_spiral_galaxy(0.5, 0.1, 0.2)
    g.set_sky_camera((0.1, 0.2, 0.3), 8, 4, 0.1)
    assert lib.cmi_gpu_dust_shoot(g._h, SEED, 0, 10) == K.ESTATE
    assert b"cell source" in lib.cmi_gpu_last_error()
    assert lib.cmi_gpu_dust_probe(g._h, E.DUST_PROBE_TRACE, SEED, 0, 1, None,
                                  SL._p(np.zeros(12)), 1) == K.ESTATE
    # after the refusal: the cell source with this camera, then with the
    # parallel one
    g.set_cell_source_field(np.ones(512))
    g.dust_shoot(SEED, 0, 1000)
    assert g.download_image()[0].sum() > 0.
    g.set_ccd_image(0.7, 0.3, 8, 8, (-2., -2.), (4., 4.))
    g.dust_shoot(SEED, 0, 1000)
    assert g.download_image().shape == (3, 8, 8)
    assert g.download_image()[0].sum() > 0.
    g.close()


# ----------------------------------------------------------- end to end --

def test_scattered_sky_map_at_albedo_0_is_the_ray_traced_one():
    """11. render_scattered_line_sky_map at albedo 0 against render_line_sky
    of the same engine (8 x 8 rays per pixel of equal solid angles, the same
    cross section): per judged pixel |I_mc - I_rt| <= 5 sqrt(sum of squared
    contributions) x scale, the variance from the restatement run on the
    device's emissivities; at least 75 % of the lit pixels have 100 hits and
    are judged. The scene is test_scattered_sky_host.py's identity (grid,
    observer, r_min, map, sigma, packets, seed). Gas of one temperature and
    ionisation emits H-alpha in proportion to the density squared; in the
    cells within r_min of the observer the density is 1e-8 of the scene's
    (a line source follows the state, so the mask goes through the state
    rather than through set_cell_source_field; the ray-traced side sees the
    same state). Their emission is then 1e-16 of the scene's per cell, not
    exactly zero: the expected number of packets from all 21 cells is 1e-11
    of 4e5, and the test asserts on the restatement that none of this run's
    direct events was excluded (hits.sum() == N)."""
    from cmacionize_amd import GpuEngine
    from test_gpu_physics import LEX
    box, model, _, mask, cam = K.identity_scene()
    density = model.density * np.where(mask > 0., 1., 1e-8)
    eng = GpuEngine(tuple(int(v) for v in model.ncell), tuple(model.anchor),
                    tuple(model.sides), (0, 0, 0), device=0)
    eng.set_abundances(LEX[1:])
    x = np.full((14, model.n), 0.3)
    x[0] = 1e-3
    eng.upload_cells(density, np.full(model.n, 8000.), x)
    w = eng.compute_emissivities(["HAlpha"])["HAlpha"]
    ratio = w / density ** 2
    assert w.min() > 0. and np.allclose(ratio, ratio[0], rtol=1e-12)
    N, seed = K.IDENTITY_PACKETS, K.IDENTITY_SEED
    args = (["HAlpha"], cam.origin, cam.nlon, cam.nlat, N, seed, model.sigma,
            0., model.g, model.p_l, cam.r_min)
    mc = eng.render_scattered_line_sky_map(*args)
    assert mc.shape == (1, 3, cam.nlon, cam.nlat)
    assert not mc[0, 1].any() and not mc[0, 2].any()
    d = K.subray_directions(cam, 8)
    rt = eng.render_line_sky(["HAlpha"], cam.origin, d.reshape(-1, 3),
                             model.sigma)["HAlpha"]
    rt = rt.reshape(cam.nlon, cam.nlat, -1).mean(axis=2)
    dark = eng.render_scattered_line_sky_map(*args, direct_light=False)
    eng.close()
    assert dark.shape == mc.shape and not dark.any()
    model.density = density
    ref = K.Restatement(model, w, cam)
    image, counters, squares, hits = ref.shoot(seed, 0, N, True)
    assert hits.sum() == N
    scale = ref.total() / N / cam.solid_angles()
    lit = rt > 0.
    judged = lit & (hits >= 100)
    assert lit.sum() == cam.nlon * cam.nlat
    assert judged.sum() >= 0.75 * lit.sum()
    z = np.abs(mc[0, 0] - rt)[judged] / \
        (np.sqrt(squares[judged]) * scale[judged])
    print("worst", z.max(), "rms", np.sqrt(np.mean(z ** 2)))
    assert z.max() <= 5.
    # the device's map is the restatement's, far inside the noise
    assert np.allclose(mc[0, 0], image[0] * scale, rtol=1e-6,
                       atol=1e-9 * rt.max())


FILE_NAMES = {"Halpha": "HAlpha", "OIII_5007": "OIII_5007"}


def test_driver_writes_the_scattered_sky_maps(tmp_path):
    """12. `cmi-gpu --emission` with `EmissionSkyMaps:scattering: true` on
    the 14^3 snapshot of the existing driver tests: three more files per
    line, equal to the Python call's result; the ray-traced file as without
    the switch."""
    import hdf5_mini
    import oracle_lib as o
    from test_gpu_physics import lexington_engine
    exe = SL.CMI_GPU
    bench = os.path.join(SL.ROOT, "benchmarks")
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

    nlon, nlat, sigma = 40, 22, 2.e-27
    observer = (5.e16, -3.e16, 2.e16)
    lon, lat = (-1., 2.), (-0.5, 1.)
    pole, zero = (0., 0., 2.), (0., 3., 1.)
    npackets, seed, albedo, g, p_l, r_min = 20000, 9, 0.54, 0.44, 0.43, 2.e16
    switches = "EmissivityValues:\n" + "".join(
        "  %s: true\n" % name for name in FILE_NAMES)
    block = ("EmissionSkyMaps:\n"
             "  observer position: [%r m, %r m, %r m]\n"
             "  number of longitude pixels: %d\n"
             "  number of latitude pixels: %d\n"
             "  longitude range: [%r radians, %r radians]\n"
             "  latitude range: [%r radians, %r radians]\n"
             "  frame pole: [%r, %r, %r]\n"
             "  frame zero longitude: [%r, %r, %r]\n"
             "  dust cross section per hydrogen: %r m^2\n"
             "  filename prefix: %%s\n  output folder: %s\n" %
             (observer + (nlon, nlat) + lon + lat + pole + zero +
              (sigma, str(tmp_path))))
    scattering = ("  scattering: true\n  number of packets: %d\n"
                  "  random seed: %d\n  dust albedo: %r\n"
                  "  dust asymmetry: %r\n"
                  "  dust peak linear polarisation: %r\n"
                  "  exclusion radius: %r m\n" %
                  (npackets, seed, albedo, g, p_l, r_min))
    (tmp_path / "plain.param").write_text(switches + block % "plain")
    (tmp_path / "mc.param").write_text(switches + block % "mc" + scattering)
    for params, file in (("plain.param", plain), ("mc.param", snapshot)):
        r = subprocess.run([exe, "--emission", "--params", params, "--file",
                            file], capture_output=True, text=True,
                           cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
    assert not [n for n in os.listdir(tmp_path) if "plain" in n and
                "scattered" in n]

    f = hdf5_mini.read(plain)
    ions = ["H", "He", "C+", "C++", "N", "N+", "N++", "O", "O+", "Ne", "Ne+",
            "S+", "S++", "S+++"]
    unit_length = 0.01 * float(np.ravel(
        f["/Units"].attrs["Unit length in cgs (U_L)"])[0])
    mid = f["/PartType0/Coordinates"].data.reshape(-1, 3) * unit_length
    idx = np.floor(ncell * mid / (10. * o.PC)).astype(np.int64)
    cell = (idx[:, 0] * ncell + idx[:, 1]) * ncell + idx[:, 2]

    def placed(values):
        out = np.empty_like(values)
        out[..., cell] = values
        return out

    eng = lexington_engine(ncell)
    eng.upload_cells(
        placed(f["/PartType0/NumberDensity"].data / unit_length ** 3),
        placed(f["/PartType0/Temperature"].data * float(np.ravel(
            f["/Units"].attrs["Unit temperature in cgs (U_T)"])[0])),
        placed(np.array([f["/PartType0/NeutralFraction" + i].data
                         for i in ions])))
    want = eng.render_scattered_line_sky_map(
        list(FILE_NAMES.values()), observer, nlon, nlat, npackets, seed,
        sigma, albedo, g, p_l, r_min, lon, lat, pole, zero)
    eng.close()
    for k, file_name in enumerate(FILE_NAMES):
        traced = open(str(tmp_path / ("mc_%s.dat" % file_name)), "rb").read()
        assert traced == open(str(tmp_path / ("plain_%s.dat" % file_name)),
                              "rb").read()
        for j, stokes in enumerate("IQU"):
            path = tmp_path / ("mc_%s_scattered_%s.dat" % (file_name, stokes))
            assert path.stat().st_size == 8 * nlon * nlat
            got = np.fromfile(str(path)).reshape(nlon, nlat)
            top = np.abs(want[k, 0]).max()
            assert top > 0.
            # the same terms, added in another order by the atomics
            assert np.allclose(got, want[k, j], rtol=1e-12,
                               atol=1e-14 * top), (file_name, stokes)
        assert np.abs(want[k, 1]).max() > 0.
