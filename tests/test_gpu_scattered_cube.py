"""GPU tests of the scattered-light line cubes (include/cmi_gpu.h,
"scattered-light line cubes"): cmi_gpu_set_scattered_cube,
cmi_gpu_download_cube_view, the CUBE instantiations of the dust kernels and
the CUBE_TRACE probe, GpuEngine.render_scattered_line_cube and
render_scattered_line_sky_map_cube - against the CPU restatement
tests/support/scattered_cube_reference.c on the same random streams (checked
on its own in test_scattered_cube_host.py) and against the identities of the
contract.

Scenes: scattered_line_lib.identity_model's 10 x 12 x 9 box, 16 x 16 pixels,
its view and sigma; the velocity field of scattered_cube_lib (a shear plus
solid rotation), widths of 8 to 12 km/s, sigma_turb 2 km/s.

Tolerance of u and b in the traces. The walk's positions and directions
agree with the restatement's to the tolerances of test_gpu_scattered_line.py
::test_traces: positions to 1e-12 of the box side, Stokes to 1e-11, weights
to rtol 1e-11; directions are not in a row, but a direction is one sin / cos
of angles that come out of the same arithmetic and is held to 1e-11 by those
columns (the weight's Henyey-Greenstein factor is a function of k . d). With
a direction error delta <= 1e-11 per event:
  u is a sum over the packet's events of terms dot3(v, k) - one at emission,
  two per completed scattering, two at the peel-off -, each off by at most
  |v| delta plus, where a position error of 1e-12 side could matter, nothing
  (the cell of a position is the same on both sides; rows on a cell wall are
  left out). Row j >= 1 of a packet is the peel-off at its j-th scattering,
  after j - 1 completed ones: |u_gpu - u_cpu| <= (1 + 2 (j - 1) + 2) vmax
  delta = (2 j + 1) vmax delta, with vmax the scene's largest speed. This is
  within what (nscatter + 1) direction errors allow. Row 0, the direct
  light, is the one term dot3(v_e, d): for the parallel camera d is the
  camera's constant and u is equal to the bit; for the point camera it is
  off by at most vmax delta. The observer's velocity adds one term of
  |v_obs| delta to every row of the point camera.
  For the point camera the direction to the observer is (o - p) / r of a
  position held to 1e-12 side with r >= r_min: delta there is 1e-11 + 1e-12
  side / r_min, used for every term.
  s2 = s2_e + 2 sigma_t^2 sum (1 - k . k') has, in row j, j - 1 terms of
  completed scatterings and the peel-off's: it is off by at most
  2 sigma_t^2 j 2 delta, and b = sqrt(2 s2) by that over b:
  |b_gpu - b_cpu| <= 4 sigma_t^2 j delta / b_min + 4 eps b (row 0: 4 eps b).
Rounding of the sums themselves (a few eps vmax) is far below both."""
import numpy as np
import pytest

import scattered_cube_lib as Q
import scattered_line_lib as SL
import scattered_sky_lib as SS
import test_gpu_dust as D
from test_gpu_dust import SEED, _on_box_face

pytestmark = pytest.mark.gpu

ALBEDO = 0.6
WIDE = 1.0e6
DELTA = 1e-11  # the direction tolerance of the traces
NCHAN = (1, 5, 8, 9, 19)
AXIS = (-4.0e4, 4.0e4)
OBSERVER_VELOCITY = np.array([1.0e3, 2.0e3, -3.0e3])


def _camera(model):
    r_min = float((model.sides / model.ncell).max())
    return SS.Camera(SS.IDENTITY_OBSERVER, 16, 16, r_min)


class Scene:
    """engine and restatement of one camera kind; `cube` sets the same cube
    mode on both"""

    def __init__(self, point, albedo=ALBEDO, sigma=None):
        self.box, self.model, self.field = SL.identity_model(albedo)
        if sigma is not None:
            self.model.sigma = sigma
        self.point = point
        self.cam = _camera(self.model) if point else None
        self.eng = SL.make_engine(self.model, self.field)
        if point:
            self.cam.apply(self.eng)
        self.velocity, self.vmax, self.shear = Q.trace_velocity(self.model)
        self.widths = Q.trace_widths(self.model)

    def moving(self, nchan, vmin, vmax, boost=None, observer_boost=None):
        v = self.velocity if boost is None else self.velocity + boost
        vo = None
        if self.point:
            vo = OBSERVER_VELOCITY if observer_boost is None else \
                OBSERVER_VELOCITY + observer_boost
        return Q.Cube(nchan, vmin, vmax, self.widths, Q.TRACE_SIGMA_TURB, v,
                      vo)

    def cube(self, q):
        q.apply(self.eng)
        return Q.Restatement(self.model, self.field, q, self.cam)

    def run(self, seed, first, n):
        """image (3, nx, ny), cube (3, nchan, nx, ny) and the counters of
        packets [first, first + n) on the device"""
        self.eng.reset_image()
        self.eng.dust_shoot(seed, first, n)
        return (self.eng.download_image(), self.eng.download_cubes()[0],
                self.eng.get_dust_counters())


@pytest.fixture(scope="module", params=[False, True], ids=["parallel", "point"])
def scene(request):
    s = Scene(request.param)
    yield s
    s.eng.close()


def _additive(a, b, scale):
    """test_additive's tolerances: the order of the atomics only"""
    return np.allclose(a, b, rtol=1e-12, atol=1e-14 * np.abs(scale).max())


# ------------------------------------------------------------- traces --

def test_traces(scene):
    """256 packets of CUBE_TRACE against the restatement: the first 8 columns
    at test_traces' tolerances, u and b at the module docstring's"""
    from cmacionize_amd import engine as E
    s = scene
    ref = s.cube(s.moving(9, *AXIS))
    n, cap = 256, 64
    gpu = s.eng.dust_probe(E.DUST_PROBE_CUBE_TRACE, Q.TRACE_SEED, 0, n, None,
                           cap)
    cpu = ref.trace(Q.TRACE_SEED, 0, n, cap)
    # the walk is the image mode's: the same rows but for the two new columns
    plain = s.eng.dust_probe(E.DUST_PROBE_TRACE, Q.TRACE_SEED, 0, n, None, cap)
    assert np.array_equal(plain[:, :4], gpu[:, :4])
    assert np.array_equal(plain[:, 4:].reshape(n, cap, 8),
                          gpu[:, 4:].reshape(n, cap, 10)[:, :, :8])
    assert np.all(gpu[:, 3] == 0.)
    assert cpu[:, 1].max() >= 3 and cpu[:, 0].max() < cap
    assert np.array_equal(gpu[:, 0], cpu[:, 0])
    side = s.model.sides.max()
    g = gpu[:, 4:].reshape(n, cap, 10)
    c = cpu[:, 4:].reshape(n, cap, 10)
    vobs = float(np.sqrt((OBSERVER_VELOCITY ** 2).sum())) if s.point else 0.
    delta = DELTA + (1e-12 * side / s.cam.r_min if s.point else 0.)
    b_min = s.widths.min()
    checked = left_out = 0
    for k in range(n):
        ev = int(cpu[k, 0])
        a, b = g[k, :ev], c[k, :ev]
        assert np.allclose(a[:, 0:3], b[:, 0:3], rtol=0., atol=1e-12 * side), k
        assert np.allclose(a[:, 3:7], b[:, 3:7], rtol=0.,
                           atol=1e-11 * np.abs(b[:, 3:4])), k
        assert np.allclose(a[:, 7], b[:, 7], rtol=1e-11, atol=0.), k
        # rows of excluded events are zeros on both sides
        seen = b[:, 9] != 0.
        assert np.array_equal(seen, a[:, 9] != 0.), k
        wall = Q.near_wall(s.model, b[:, 0:3])
        left_out += int(wall.sum())
        # row j >= 1 is the peel-off at the j-th scattering (the direct
        # light first; with the direct light every packet has it)
        j = np.arange(ev)
        tol_u = (2. * j + 1.) * s.vmax * delta + vobs * delta
        if not s.point:
            tol_u[0] = 0.  # 4.12's u, bit for bit
        tol_b = 4. * Q.TRACE_SIGMA_TURB ** 2 * j * delta / b_min + \
            4. * np.finfo(float).eps * b[:, 9]
        keep = seen & ~wall
        assert np.all(np.abs(a[keep, 8] - b[keep, 8]) <= tol_u[keep]), k
        assert np.all(np.abs(a[keep, 9] - b[keep, 9]) <= tol_b[keep]), k
        checked += int(keep.sum())
    assert left_out == 0  # the seed was chosen so (checked on the CPU)
    assert checked > 400
    # u and b are not constants of the scene
    rows = Q.events(cpu, cap)
    rows = rows[rows[:, 9] != 0.]
    assert np.ptp(rows[:, 8]) > 5.0e3 and np.ptp(rows[:, 9]) > 2.0e3


def test_traces_past_one_launch(scene):
    """The cube instantiations of the probe kernel (they serve CUBE_TRACE
    alone) with more rows than one launch of cmi_gpu_dust_probe takes (2^14):
    the rows past it are the rows traced alone, with first_packet moved up by
    2^14."""
    from cmacionize_amd import engine as E
    s = scene
    s.cube(s.moving(9, *AXIS))
    launch, cap = 1 << 14, 2
    gpu = s.eng.dust_probe(E.DUST_PROBE_CUBE_TRACE, SEED, 3, launch + 50, None,
                           cap)
    alone = s.eng.dust_probe(E.DUST_PROBE_CUBE_TRACE, SEED, 3 + launch, 50,
                             None, cap)
    assert gpu[launch:, 0].min() >= 1.
    assert np.array_equal(gpu[launch:], alone)


def test_a_packet_alone_is_the_packet_among_others(scene):
    """the guard of DESIGN.md 4.6 for the new instantiations"""
    from cmacionize_amd import engine as E
    s = scene
    s.cube(s.moving(9, *AXIS))
    cap = 64
    among = s.eng.dust_probe(E.DUST_PROBE_CUBE_TRACE, SEED, 0, 64, None, cap)
    assert among[:, 1].max() >= 2
    for k in (0, 1, 17, 31, 32, 63, int(np.argmax(among[:, 1]))):
        alone = s.eng.dust_probe(E.DUST_PROBE_CUBE_TRACE, SEED, k, 1, None,
                                 cap)[0]
        assert np.array_equal(alone, among[k]), k


# --------------------------------------------------------- whole runs --

def _bad_elements(gpu, cpu, image):
    """elements of the cube off by more than 1e-9 of the restatement's pixel
    summed over the channels (a channel's share is a difference of two erf
    values, so the pixel is the scale); Q and U are signed sums whose pixel
    can cancel and get, as in test_gpu_dust._bad_pixels, 1e-12 of the
    image's largest |I| on top - I does not"""
    scale = np.abs(cpu.sum(axis=1, keepdims=True))
    floor = np.array([0., 1., 1.]).reshape(3, 1, 1, 1) * \
        (1e-12 * np.abs(image[0]).max())
    return np.abs(gpu - cpu) > 1e-9 * scale + floor


def _culprits(s, ref, lo, hi, mask, out):
    image, cube, _ = s.run(SEED, lo, hi - lo)
    cimage, ccube, _ = ref.shoot(SEED, lo, hi - lo)
    if not np.any(_bad_elements(cube, ccube, cimage) & mask):
        return
    if hi - lo == 1:
        out.append(lo)
        return
    mid = (lo + hi) // 2
    _culprits(s, ref, lo, mid, mask, out)
    _culprits(s, ref, mid, hi, mask, out)


def _is_threshold_case(s, gt, ct, cap):
    """a culprit's traces: an event on a pixel edge or a different number of
    events as the image's tests accept them, or a position on a cell wall
    (the scattering cell, hence u, may then differ)"""
    g = gt[4:].reshape(cap, 10)
    c = ct[4:].reshape(cap, 10)
    n = int(min(gt[0], ct[0], cap))
    if Q.near_wall(s.model, c[:n, 0:3]).any():
        return True
    g8 = np.r_[gt[:4], g[:, :8].ravel()]
    c8 = np.r_[ct[:4], c[:, :8].ravel()]
    d = s.model.describe()
    if s.point:
        import test_gpu_scattered_sky as T
        ref = SS.Restatement(s.model, s.field, s.cam)
        return T._is_threshold_case(d, s.cam, ref, g8, c8, cap)
    ref = SL.Restatement(s.model, s.field)
    return D._is_threshold_case(d, ref, g8, c8, cap)


def test_whole_run(scene):
    """test_whole_run's scheme on the cube: 5e4 packets, elements off by more
    than the bound are traced to their packets by bisection and those shown
    to be threshold cases; the run without them then agrees. The image of the
    run is the image mode's."""
    from cmacionize_amd import engine as E
    s = scene
    N = 50000
    s.eng.set_scattered_cube(0, 0., 1.)
    s.eng.reset_image()
    s.eng.dust_shoot(SEED, 0, N)
    plain = s.eng.download_image()
    plain_atomics = s.eng.get_dust_counters()["natomics"]
    ref = s.cube(s.moving(19, *AXIS))
    image, cube, c = s.run(SEED, 0, N)
    assert _additive(image, plain, plain[0])
    cimage, ccube, cc = ref.shoot(SEED, 0, N)
    assert c["npackets"] == N and c["ncapped"] == 0 and cc[2] == 0
    assert cc[1] > N and np.count_nonzero(ccube[0]) > 1000
    assert np.abs(ccube[1]).max() > 0. and np.abs(ccube[2]).max() > 0.
    # every cube atomic is counted
    assert c["natomics"] > 5 * plain_atomics
    bad = _bad_elements(cube, ccube, cimage)
    print("differing elements", int(bad.sum()), "worst",
          (np.abs(cube - ccube) /
           (np.abs(ccube.sum(axis=1, keepdims=True)) + 1e-300)).max())
    if not np.any(bad):
        assert c["nscatter"] == cc[1] and c["nsteps"] == cc[0]
        return
    culprits = []
    _culprits(s, ref, 0, N, bad, culprits)
    assert culprits, "differing elements without a differing packet"
    cap = 4096
    for k in culprits:
        gt = s.eng.dust_probe(E.DUST_PROBE_CUBE_TRACE, SEED, k, 1, None,
                              cap)[0]
        ct = ref.trace(SEED, k, 1, cap)[0]
        ref.setup()
        assert _is_threshold_case(s, gt, ct, cap), k
        ref.setup()
    ok = np.ones(N, bool)
    ok[culprits] = False
    shape = cube.shape
    gpu2, cpu2, img2 = np.zeros(shape), np.zeros(shape), np.zeros((3,) +
                                                                  shape[2:])
    edges = np.flatnonzero(np.diff(np.r_[0, ok.astype(int), 0]))
    for lo, hi in zip(edges[0::2], edges[1::2]):
        gpu2 += s.run(SEED, int(lo), int(hi - lo))[1]
        ci, cq, _ = ref.shoot(SEED, int(lo), int(hi - lo))
        cpu2 += cq
        img2 += ci
    assert not np.any(_bad_elements(gpu2, cpu2, img2))


@pytest.mark.parametrize("n", [3, 67])
def test_a_few_lanes(scene, n):
    """3 packets are 3 active lanes of one wave, 67 a full wave and 3 lanes
    of the next: the deposit under a partial mask"""
    s = scene
    ref = s.cube(s.moving(9, *AXIS))
    image, cube, c = s.run(SEED, 1000, n)
    cimage, ccube, cc = ref.shoot(SEED, 1000, n)
    assert c["npackets"] == n and np.count_nonzero(ccube[0]) >= n
    assert c["nscatter"] == cc[1]
    assert not np.any(_bad_elements(cube, ccube, cimage))
    assert np.allclose(image, cimage, rtol=1e-9,
                       atol=1e-12 * np.abs(cimage[0]).max())


def test_additive(scene):
    s = scene
    s.cube(s.moving(9, *AXIS))
    N, a = 30000, 12345
    whole_image, whole, _ = s.run(SEED, 0, N)
    s.eng.reset_image()
    s.eng.dust_shoot(SEED, 0, a)
    s.eng.dust_shoot(SEED, a, N - a)
    parts = s.eng.download_cubes()[0]
    c = s.eng.get_dust_counters()
    assert c["ncapped"] == 0 and c["npackets"] == N
    assert _additive(parts, whole, whole_image[0])
    # reset_image zeroes the cubes
    s.eng.reset_image()
    assert not s.eng.download_cubes().any()


# --------------------------------------------------------- identities --

def test_one_covering_channel_is_the_image(scene):
    """1."""
    s = scene
    s.cube(s.moving(1, -WIDE, WIDE))
    image, cube, _ = s.run(SEED, 0, 20000)
    assert np.abs(image[1]).max() > 0.
    assert _additive(cube[:, 0], image, image[0])


@pytest.mark.parametrize("nchan", NCHAN[1:])
def test_covering_channels_sum_to_the_image(scene, nchan):
    """2."""
    s = scene
    s.cube(s.moving(nchan, -WIDE, WIDE))
    image, cube, _ = s.run(SEED, 0, 20000)
    assert _additive(cube.sum(axis=1), image, image[0])
    s.cube(s.moving(nchan, *AXIS))
    image2, cube2, _ = s.run(SEED, 0, 20000)
    assert _additive(image2, image, image[0])
    assert np.count_nonzero(cube2[0].sum(axis=(1, 2))) == nchan


def test_gas_at_rest_with_one_width(scene):
    """4."""
    s = scene
    nchan, b = 8, 9.0e3
    q = Q.Cube(nchan, -2.0e4, 2.4e4, np.full(s.model.n, b))
    ref = s.cube(q)
    image, cube, _ = s.run(SEED, 0, 20000)
    f = ref.shares(0., b)
    # (the device's erf is within 2 ulps of the host's: 1e-12 of a share of
    # 1e-3 and more is a thousand times that)
    assert f.min() > 1e-3
    assert _additive(cube, image[:, None] * f[None, :, None, None], image[0])


@pytest.mark.parametrize("point", [False, True], ids=["parallel", "point"])
def test_galilean_identity_with_several_scatterings(point):
    """3. albedo 0.9 and optical depths of 3 to 10: more than two scatterings
    per packet. Parallel: V on every cell and the axis shifted by -dot3(V,
    d); point: V on every cell and on the observer. The bound is
    test_scattered_cube_host.py's: 1e-9 of the image's pixel."""
    s = Scene(point, albedo=0.9, sigma=0.25)
    try:
        N = 20000
        V = np.array([-5.0e3, 9.0e3, 6.0e3])
        s.cube(s.moving(9, -3.0e4, 3.0e4))
        image, cube, c = s.run(SEED, 0, N)
        assert c["nscatter"] / N > 2.
        if point:
            s.cube(s.moving(9, -3.0e4, 3.0e4, V, V))
        else:
            m = s.model
            d = np.array([np.sin(m.theta) * np.cos(m.phi),
                          np.sin(m.theta) * np.sin(m.phi), np.cos(m.theta)])
            shift = -float(V @ d)
            s.cube(s.moving(9, -3.0e4 + shift, 3.0e4 + shift, V))
        image_b, cube_b, _ = s.run(SEED, 0, N)
        assert _additive(image_b, image, image[0])
        assert np.allclose(cube_b, cube, rtol=0.,
                           atol=1e-9 * np.abs(image[:, None]) + 1e-300)
        # not trivially: the boost alone changes the cube
        s.cube(s.moving(9, -3.0e4, 3.0e4, V))
        cube_c = s.run(SEED, 0, N)[1]
        assert not np.allclose(cube_c, cube, rtol=1e-3, atol=0.)
    finally:
        s.eng.close()


# -------------------------------------------------------------- views --

@pytest.mark.parametrize("point", [False, True], ids=["parallel", "point"])
def test_views_are_the_single_cameras(point):
    """view k of a 3-view run is the single camera's run of the same seed"""
    box, model, field = SL.identity_model(ALBEDO)
    eng = SL.make_engine(model, field)
    v, _, _ = Q.trace_velocity(model)
    eng.set_cell_velocities(v.T.copy())
    widths = Q.trace_widths(model)
    N = 20000
    vo = np.array([OBSERVER_VELOCITY, -OBSERVER_VELOCITY, [0., 5.0e3, 0.]])
    if point:
        origins = np.array([SS.IDENTITY_OBSERVER, (0.9, 1.3, 2.4),
                            (-0.4, 3.0, 3.9)])
        r_min = float((model.sides / model.ncell).max())

        def views():
            eng.set_sky_cameras(origins, 16, 16, r_min)

        def single(k):
            eng.set_sky_camera(origins[k], 16, 16, r_min)
    else:
        theta = [model.theta, 0.4, 2.0]
        phi = [model.phi, 2.5, -1.0]

        def views():
            eng.set_ccd_images(theta, phi, 16, 16, model.img_anchor,
                               model.img_sides)

        def single(k):
            eng.set_ccd_image(theta[k], phi[k], 16, 16, model.img_anchor,
                              model.img_sides)
    try:
        views()
        eng.set_scattered_cube(9, *AXIS, Q.TRACE_SIGMA_TURB, widths, vo)
        eng.dust_shoot(SEED, 0, N)
        images = eng.download_images()
        cubes = eng.download_cubes()
        per_view = [eng.get_dust_view_counters(k)["natomics"]
                    for k in range(3)]
        assert cubes.shape == (3, 3, 9, 16, 16)
        assert sum(per_view) == eng.get_dust_counters()["natomics"]
        for k in range(3):
            single(k)
            eng.set_scattered_cube(9, *AXIS, Q.TRACE_SIGMA_TURB, widths,
                                   vo[k:k + 1])
            eng.dust_shoot(SEED, 0, N)
            assert eng.get_dust_counters()["natomics"] == per_view[k]
            image = eng.download_image()
            assert image[0].any()
            assert _additive(images[k], image, image[0])
            assert _additive(cubes[k], eng.download_cubes()[0], image[0])
        assert not _additive(cubes[0], cubes[1], images[0, 0])
    finally:
        eng.close()


# ----------------------------------------------------------- refusals --

def test_refusals_leave_a_usable_engine():
    from cmacionize_amd import engine as E
    from test_gpu_physics import LEX
    box, model, field = SL.identity_model(ALBEDO)
    eng = SL.make_engine(model, field)
    lib = eng._lib
    h = eng._h
    widths = Q.trace_widths(model)
    w = SL._p(widths)

    def works():
        eng.reset_image()
        eng.dust_shoot(SEED, 0, 2000)
        cube = eng.download_cubes()[0]
        assert cube.shape == (3, 5, 16, 16)
        assert _additive(cube.sum(axis=1), eng.download_image(),
                         cube[0].sum(axis=0))

    try:
        # no cube mode yet
        with pytest.raises(E.EngineError, match="cube mode is not set"):
            eng.download_cubes()
        assert lib.cmi_gpu_download_cube_view(h, 0, None, None, None) == \
            SL.ESTATE
        assert lib.cmi_gpu_dust_probe(h, E.DUST_PROBE_CUBE_TRACE, SEED, 0, 1,
                                      None, SL._p(np.zeros(4)), 0) == SL.ESTATE
        eng.set_scattered_cube(5, -WIDE, WIDE, 0., widths)
        works()
        # bad arguments: the previous cube mode stays
        for args in ((-1, -1., 1., 0., w, None), (5, 1., 1., 0., w, None),
                     (5, 2., 1., 0., w, None), (5, -np.inf, 1., 0., w, None),
                     (5, -1., 1., -1., w, None), (5, -1., 1., np.nan, w, None),
                     ((1 << 28) // 256 + 1, -1., 1., 0., w, None)):
            assert lib.cmi_gpu_set_scattered_cube(h, *args) == SL.EINVAL, args
            works()
        bad = widths.copy()
        bad[7] = -1.
        assert lib.cmi_gpu_set_scattered_cube(h, 5, -1., 1., 0., SL._p(bad),
                                              None) == SL.EINVAL
        assert b"negative or not finite" in lib.cmi_gpu_last_error()
        bad[7] = np.inf
        assert lib.cmi_gpu_set_scattered_cube(h, 5, -1., 1., 0., SL._p(bad),
                                              None) == SL.EINVAL
        vo = np.array([0., np.nan, 0.])
        assert lib.cmi_gpu_set_scattered_cube(h, 5, -1., 1., 0., w,
                                              SL._p(vo)) == SL.EINVAL
        # a field source needs widths
        assert lib.cmi_gpu_set_scattered_cube(h, 5, -1., 1., 0., None,
                                              None) == SL.ESTATE
        works()
        assert lib.cmi_gpu_download_cube_view(h, 1, None, None, None) == \
            SL.EINVAL
        # stale: the velocities, the source, the camera
        for change in (
                lambda: eng.set_cell_velocities(np.zeros((3, model.n))),
                lambda: eng.set_cell_velocities(None),
                lambda: eng.set_cell_source_field(field),
                lambda: eng.set_ccd_image(model.theta, model.phi, 16, 16,
                                          model.img_anchor, model.img_sides)):
            change()
            assert lib.cmi_gpu_dust_shoot(h, SEED, 0, 10) == SL.ESTATE
            assert b"set_scattered_cube again" in lib.cmi_gpu_last_error()
            assert lib.cmi_gpu_dust_probe(h, E.DUST_PROBE_TRACE, SEED, 0, 1,
                                          None, SL._p(np.zeros(4)), 0) == \
                SL.ESTATE
            eng.set_scattered_cube(5, -WIDE, WIDE, 0., widths)
            works()
        # the galaxy has no line (identity_model's box does not hold the
        # origin, so the galaxy is set on a box that does)
        eng.set_scattered_cube(0, 0., 1.)
        eng.reset_image()
        eng.dust_shoot(SEED, 0, 100)
        assert eng.download_image()[0].any()
    finally:
        eng.close()

    from cmacionize_amd import GpuEngine
    n = 8
    gal = GpuEngine((n, n, n), (-1e17,) * 3, (2e17,) * 3, (0, 0, 0), device=0)
    try:
        gal.set_abundances(LEX[1:])
        x = np.full((14, n ** 3), 0.3)
        x[0] = 1e-3
        gal.upload_cells(np.full(n ** 3, 1e8), np.full(n ** 3, 8000.), x)
        gal.set_dust_scattering_per_hydrogen(0.4, 0.3, 0.5, 1e-27)
        gal.set_ccd_image(0.7, 0.3, 8, 8, (-2e17, -2e17), (4e17, 4e17))
        gl, gh = gal._lib, gal._h
        # no source at all, then the galaxy
        assert gl.cmi_gpu_set_scattered_cube(gh, 5, -1e5, 1e5, 0., None,
                                             None) == SL.ESTATE
        gal.set_continuous_source_spiral_galaxy(1e17, 1e16, 0.2)
        assert gl.cmi_gpu_set_scattered_cube(gh, 5, -1e5, 1e5, 0., None,
                                             None) == SL.ESTATE
        assert b"no line" in gl.cmi_gpu_last_error()
        # a blended entry is not the line of one ion; widths are refused
        for blend in ("HII", "BALMER_JUMP_LOW", "Hrec_s"):
            try:
                gal.set_cell_source_line(blend)
                break
            except E.EngineError:  # (an entry that emits nothing here)
                continue
        assert gl.cmi_gpu_set_scattered_cube(gh, 5, -1e5, 1e5, 0., None,
                                             None) == SL.EINVAL
        assert b"not the line of one ion" in gl.cmi_gpu_last_error()
        gal.set_cell_source_line("HAlpha")
        ones = np.ones(n ** 3)
        assert gl.cmi_gpu_set_scattered_cube(gh, 5, -1e5, 1e5, 0.,
                                             SL._p(ones), None) == SL.ESTATE
        gal.set_scattered_cube(5, -1e5, 1e5, 1e3)
        gal.dust_shoot(SEED, 0, 2000)
        cube = gal.download_cubes()[0]
        image = gal.download_image()
        assert _additive(cube.sum(axis=1), image, image[0])
        # a line source is stale once the cells change
        gal.upload_cells(np.full(n ** 3, 1e8), np.full(n ** 3, 9000.), x)
        assert gl.cmi_gpu_dust_shoot(gh, SEED, 0, 10) == SL.ESTATE
        assert gl.cmi_gpu_set_scattered_cube(gh, 5, -1e5, 1e5, 0., None,
                                             None) == SL.ESTATE
        assert b"cells changed" in gl.cmi_gpu_last_error()
        gal.set_cell_source_line("HAlpha")
        assert gl.cmi_gpu_dust_shoot(gh, SEED, 0, 10) == SL.ESTATE
        gal.set_scattered_cube(5, -1e5, 1e5, 1e3)
        gal.dust_shoot(SEED, 0, 2000)
        assert gal.download_cubes().any()
        # switching back to the galaxy makes cube mode stale as well
        gal.set_continuous_source_spiral_galaxy(1e17, 1e16, 0.2)
        assert gl.cmi_gpu_dust_shoot(gh, SEED, 0, 10) == SL.ESTATE
        gal.set_scattered_cube(0, 0., 1.)
        gal.reset_image()
        gal.dust_shoot(SEED, 0, 2000)
        assert gal.download_image()[0].any()
    finally:
        gal.close()


# --------------------------------------------------------- end to end --

def _line_engine(model, density):
    from cmacionize_amd import GpuEngine
    from test_gpu_physics import LEX
    eng = GpuEngine(tuple(int(v) for v in model.ncell), tuple(model.anchor),
                    tuple(model.sides), (0, 0, 0), device=0)
    eng.set_abundances(LEX[1:])
    x = np.full((14, model.n), 0.3)
    x[0] = 1e-3
    eng.upload_cells(density, np.full(model.n, 8000.), x)
    return eng


def _judge(mc, rt, squares, hits, scale):
    lit = rt > 1e-6 * rt.max()
    judged = lit & (hits >= 100)
    assert lit.sum() > 100 and judged.sum() >= 0.75 * lit.sum()
    z = np.abs(mc - rt)[judged] / (np.sqrt(squares) * scale)[judged]
    print("worst", z.max(), "rms", np.sqrt(np.mean(z ** 2)))
    assert z.max() <= 5.


H_ALPHA_WIDTH = np.sqrt(2. * Q.BOLTZMANN * 8000. /
                        (Q.HYDROGEN * Q.ATOMIC_MASS_UNIT))


def test_scattered_cube_at_albedo_0_is_the_ray_traced_one():
    """5. render_scattered_line_cube at albedo 0 against render_line_cube of
    the same engine (supersample 8) per pixel and channel at 5 sigma, the
    variance from the restatement's addends; test_gpu_scattered_line.py's
    albedo-0 scene and its 4e5 packets, with the trace scene's velocities"""
    box, model, _ = SL.identity_model()
    eng = _line_engine(model, model.density)
    w = eng.compute_emissivities(["HAlpha"])["HAlpha"]
    v, _, _ = Q.trace_velocity(model)
    eng.set_cell_velocities(v.T.copy())
    N, seed = SL.IDENTITY_PACKETS, SL.IDENTITY_SEED
    nchan, vmin, vmax = 8, -3.2e4, 3.2e4
    args = (model.theta, model.phi, model.nx, model.ny, model.img_anchor,
            model.img_sides)
    images, cubes = eng.render_scattered_line_cube(
        ["HAlpha"], *args, N, seed, model.sigma, 0., model.g, model.p_l,
        nchan, vmin, vmax)
    assert images.shape == (1, 3, 16, 16) and cubes.shape == (1, 3, 8, 16, 16)
    assert not cubes[0, 1].any() and not cubes[0, 2].any()
    rt = eng.render_line_cube(["HAlpha"], *args, nchan, vmin, vmax, 8,
                              model.sigma)["HAlpha"]
    plain = eng.render_scattered_line_images(["HAlpha"], *args, N, seed,
                                             model.sigma, 0., model.g,
                                             model.p_l)
    eng.close()
    assert _additive(images, plain, plain[0, 0])
    q = Q.Cube(nchan, vmin, vmax, np.full(model.n, H_ALPHA_WIDTH), 0., v)
    ref = Q.Restatement(model, w, q)
    cimage, ccube, _, squares, hits = ref.shoot(seed, 0, N, True)
    total = np.zeros(1)
    Q.lib().slref_get_tables(Q._p(total), None, None)
    scale = float(total[0]) / (N * model.pixel_area)
    _judge(cubes[0, 0], rt, squares, hits, scale)
    assert np.allclose(cubes[0, 0], ccube[0] * scale, rtol=1e-6,
                       atol=1e-9 * rt.max())


def test_scattered_sky_cube_at_albedo_0_is_the_ray_traced_one():
    """5. render_scattered_line_sky_map_cube against
    render_line_sky_map_cube's rays (8 x 8 per pixel of equal solid angle),
    test_gpu_scattered_sky.py's albedo-0 scene, an observer that moves"""
    box, model, _, mask, cam = SS.identity_scene()
    density = model.density * np.where(mask > 0., 1., 1e-8)
    eng = _line_engine(model, density)
    w = eng.compute_emissivities(["HAlpha"])["HAlpha"]
    v, _, _ = Q.trace_velocity(model)
    eng.set_cell_velocities(v.T.copy())
    vo = np.array([4.0e3, -6.0e3, 2.0e3])
    N, seed = SS.IDENTITY_PACKETS, SS.IDENTITY_SEED
    nchan, vmin, vmax = 8, -3.2e4, 3.2e4
    images, cubes = eng.render_scattered_line_sky_map_cube(
        ["HAlpha"], cam.origin, cam.nlon, cam.nlat, N, seed, model.sigma, 0.,
        model.g, model.p_l, cam.r_min, nchan, vmin, vmax,
        observer_velocity=vo)
    assert cubes.shape == (1, 3, nchan, cam.nlon, cam.nlat)
    d = SS.subray_directions(cam, 8)
    rt = eng.render_line_sky_cube(["HAlpha"], cam.origin, d.reshape(-1, 3),
                                  nchan, vmin, vmax,
                                  dust_cross_section=model.sigma,
                                  observer_velocity=vo)["HAlpha"]
    rt = rt.reshape(nchan, cam.nlon, cam.nlat, -1).mean(axis=3)
    eng.close()
    model.density = density
    q = Q.Cube(nchan, vmin, vmax, np.full(model.n, H_ALPHA_WIDTH), 0., v, vo)
    ref = Q.Restatement(model, w, q, cam)
    cimage, ccube, c, squares, hits = ref.shoot(seed, 0, N, True)
    total = np.zeros(1)
    Q.lib().slref_get_tables(Q._p(total), None, None)
    scale = (float(total[0]) / N / cam.solid_angles())[None]
    _judge(cubes[0, 0], rt, squares, hits, scale)
    assert np.allclose(cubes[0, 0], ccube[0] * scale, rtol=1e-6,
                       atol=1e-9 * rt.max())
