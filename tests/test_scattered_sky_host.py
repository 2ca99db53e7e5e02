"""The CPU restatement of the scattered-light sky maps
(tests/support/scattered_sky_reference.c) on its own, the host's refusals and
the driver's new keys - no GPU: the Monte Carlo map at albedo 0 against the
ray-traced restatement (sky_image_lib.render), flux conservation, the
exclusion and window counters, the same packets as the parallel camera, the
polarisation pattern around a point source in two frames (which pins the
sign of the rotation of Q, U to the frame's pole), cmi_gpu_check_sky_camera,
`cmi-gpu --emission` with the scattering keys of EmissionSkyMaps."""
import os
import subprocess

import numpy as np
import pytest

import scattered_line_lib as SL
import scattered_sky_lib as K
import sky_image_lib as SI

DEG = np.pi / 180.


def test_monte_carlo_at_albedo_0_is_the_ray_traced_map():
    """1. Statistical identity. At albedo 0 only the direct light reaches the
    map, and its expectation per pixel is the mean of the ray-traced surface
    brightness over the pixel, with extinction n sigma. Per judged pixel
    |I_mc - I_rt| <= 5 sqrt(sum of squared contributions) x scale, scale =
    L_total / (N omega_pixel).

    Chosen values (scattered_sky_lib.identity_scene): identity_model's 10 x
    12 x 9 grid and sigma; the observer (0.3, 2.1, 3.2), inside the box and
    off every cell wall; r_min = 0.25, the longest cell side; the field
    density^2 is zeroed in the 21 cells that have a point within r_min of the
    observer, so no emission is excluded and a contribution is at most
    0.25 / (pi r_min^2). The observer sits in the box, so every pixel of the
    full sky is lit; 24 x 12 pixels and scattered_line_lib's IDENTITY_PACKETS
    = 4e5 packets give the restatement 88 .. 4000 hits per pixel, 286 of the
    288 lit pixels with 100 and more (1.6e6 packets would judge all 288 and
    change nothing else; the smaller run keeps the test short). The
    ray-traced side is 8 x 8 rays per pixel, uniform in longitude and in
    sin(latitude): equal solid angles, a plain mean. Scatterings happen
    (unseen: weight 0), and those nearer than r_min are counted as
    excluded."""
    box, model, field, mask, cam = K.identity_scene()
    assert (mask == 0.).sum() > 0
    # the observer is off every cell wall
    f = (np.array(K.IDENTITY_OBSERVER) - model.anchor) / \
        (model.sides / model.ncell)
    assert np.all(np.abs(f - np.round(f)) > 0.05)
    ref = K.Restatement(model, field, cam)
    N = K.IDENTITY_PACKETS
    image, counters, squares, hits = ref.shoot(K.IDENTITY_SEED, 0, N, True)
    assert counters[1] > 0 and counters[2] == 0 and counters[5] == 0
    assert not image[1].any() and not image[2].any()
    # no direct light was excluded: every packet's direct event was binned
    assert hits.sum() == N
    scale = ref.total() / N / cam.solid_angles()
    d = K.subray_directions(cam, 8)
    rt = SI.render(box, field, cam.origin, d.reshape(-1, 3),
                   extinction=model.density * model.sigma)[0]
    rt = rt.reshape(cam.nlon, cam.nlat, -1).mean(axis=2)
    lit = rt > 0.
    judged = lit & (hits >= 100)
    print("lit", lit.sum(), "judged", judged.sum(), "min hits",
          hits[lit].min())
    assert lit.sum() == cam.nlon * cam.nlat
    assert judged.sum() >= 0.75 * lit.sum()
    z = np.abs(image[0] * scale - rt)[judged] / \
        (np.sqrt(squares[judged]) * scale[judged])
    print("worst", z.max(), "rms", np.sqrt(np.mean(z ** 2)))
    assert z.max() <= 5.
    # an identity, not a loose bound: z is of order one
    assert 0.5 < np.sqrt(np.mean(z ** 2)) < 1.5


def test_flux_conservation():
    """2. One emitting cell, no dust, the observer outside the box, r_min =
    0: every packet's direct light lands in the full-sky map with 0.25 / (pi
    r^2), whatever its pixel."""
    n = 6 * 5 * 4
    model = SL.Model((0., 0., 0.), (1.2, 1., 0.8), (6, 5, 4), np.ones(n), 0.,
                     0.5, 0.4, 0.3, 0.7, 0.3, 8, 8, (-1., -1.), (2., 2.))
    field = np.zeros(n)
    field[57] = 2.
    cam = K.Camera((2.3, -0.7, 1.9), 16, 8, 0.)
    ref = K.Restatement(model, field, cam)
    N = 20000
    image, counters = ref.shoot(5, 0, N)
    assert counters[1] == 0 and counters[4] == 0 and counters[5] == 0
    rows = K.events(ref.trace(5, 0, N, 2), 2)
    assert len(rows) == N
    v = cam.origin - rows[:, :3]
    r2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    want = (0.25 / (np.pi * r2)).sum()
    assert abs(image[0].sum() - want) <= 1e-12 * want
    assert not image[1].any() and not image[2].any()


def _by_hand(ref, rows, cam):
    """the map of trace rows binned one by one, and their pixels"""
    ref.setup()
    image = np.zeros((3, cam.nlon * cam.nlat))
    pixels = np.array([ref.pixel(r[:3]) for r in rows])
    for r, px in zip(rows, pixels):
        if px >= 0:
            image[:, px] += r[7] * r[3:6]
    return image.reshape(3, cam.nlon, cam.nlat), pixels


def test_exclusion_and_window_counters():
    """3. An observer inside an emitting, scattering region: events nearer
    than r_min are counted and add nothing - the map is that of the same run
    without an exclusion radius with those events taken out of its trace by
    hand; with a window of half the sky the events outside it are counted,
    and they, the binned and the excluded ones are all events."""
    _, model, field = SL.identity_model(albedo=0.6)
    r_min, N, ME = 0.25, 8000, 40
    cam = K.Camera(K.IDENTITY_OBSERVER, 12, 6, r_min)
    ref = K.Restatement(model, field, cam)
    image, counters, squares, hits = ref.shoot(9, 0, N, True)
    assert counters[4] > 0 and counters[5] == 0
    # every event: the same packets without the exclusion radius
    everything = K.Restatement(model, field, K.Camera(
        K.IDENTITY_OBSERVER, 12, 6, 0.))
    rows = K.events(everything.trace(9, 0, N, ME), ME)
    v = cam.origin - rows[:, :3]
    r2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    near = r2 < r_min * r_min
    assert near.sum() == counters[4]
    by_hand, pixels = _by_hand(ref, rows[~near], cam)
    assert (pixels >= 0).all()
    assert np.allclose(image, by_hand, rtol=1e-12, atol=0.)
    assert hits.sum() == (~near).sum()
    # the trace of the run with the radius has a row of zeros for each
    with_radius = K.events(ref.trace(9, 0, N, ME), ME)
    assert np.array_equal(with_radius[:, :3], rows[:, :3])
    assert np.array_equal(with_radius[:, 7] == 0., near)
    assert not with_radius[near][:, 3:].any()
    assert np.array_equal(with_radius[~near], rows[~near])
    # half the sky
    half = K.Camera(K.IDENTITY_OBSERVER, 6, 6, r_min,
                    lon=(-0.5 * np.pi, 0.5 * np.pi))
    ref = K.Restatement(model, field, half)
    image, counters, squares, hits = ref.shoot(9, 0, N, True)
    assert counters[5] > 0
    assert counters[5] + hits.sum() + counters[4] == len(rows)
    by_hand, pixels = _by_hand(ref, rows[~near], half)
    assert (pixels == -1).sum() == counters[5]
    assert np.allclose(image, by_hand, rtol=1e-12, atol=0.)


def test_same_packets_as_the_parallel_camera():
    """4. The camera draws no random number: event for event the positions
    are the parallel camera's."""
    _, model, field = SL.identity_model(albedo=0.6)
    cam = K.Camera(K.IDENTITY_OBSERVER, 12, 6, 0.25,
                   frame=K.frame_of((0.2, -0.4, 0.8), (1., 0.3, 0.)))
    ref = K.Restatement(model, field, cam)
    point = ref.trace(21, 100, 3000, 30)
    parallel = ref.parallel_trace(21, 100, 3000, 30)
    # events, scatterings and caps (the steps differ: the march to the
    # observer is shorter than the one to the box edge)
    assert np.array_equal(point[:, [0, 1, 3]], parallel[:, [0, 1, 3]])
    assert (point[:, 2] < parallel[:, 2]).any()
    a = point[:, 4:].reshape(3000, 30, 8)
    b = parallel[:, 4:].reshape(3000, 30, 8)
    assert point[:, 0].max() > 5
    assert np.array_equal(a[:, :, :3], b[:, :, :3])


# one emitting cell in a unit box of optically thin dust, seen from inside
PATTERN_NCELL = (8, 8, 8)
PATTERN_SOURCE = (5, 4, 3)
PATTERN_OBSERVER = np.array([0.21, 0.33, 0.47])
PATTERN_PACKETS = 200000
PATTERN_G = 0.01


def _pattern_model():
    n = int(np.prod(PATTERN_NCELL))
    model = SL.Model((0., 0., 0.), (1., 1., 1.), PATTERN_NCELL, np.ones(n),
                     0.2, 1., PATTERN_G, 0.5, 0.7, 0.3, 64, 64, (-1., -1.),
                     (2., 2.))
    field = np.zeros(n)
    i, j, k = PATTERN_SOURCE
    field[(i * PATTERN_NCELL[1] + j) * PATTERN_NCELL[2] + k] = 1.
    centre = (np.array(PATTERN_SOURCE) + 0.5) / np.array(PATTERN_NCELL)
    return model, field, centre


def _band(q):
    """sum and standard deviation (from the squared contributions)"""
    return q.sum(), np.sqrt((q * q).sum())


def test_polarisation_pattern_pins_the_rotation():
    """5. Light of a point source scattered once is polarised at right
    angles to the scattering plane: tangentially around the source on the
    sky. With e_1 towards the source, Q (referred to the frame's pole) has
    one sign left and right of it (the equatorial band |b| < 10 deg, 20 deg <
    |l| < 60 deg) and the other above and below (the meridian band |l| < 10
    deg, 20 deg < |b| < 60 deg), in any frame with that e_1. Two poles: one
    perpendicular to e_1 near z, and that turned by 30 degrees about e_1,
    where a rotation of the wrong sign would turn Q by 4 chi = 120 degrees:
    flip it and leave |U| > |Q|.

    Chosen values: an 8^3 unit box of unit density, sigma = 0.2 (tau = 0.2
    across the box), albedo 1, p_l = 0.5, direct light off, g = 0.01 - the
    phase function's constants hold 1 / 2g, so g = 0 itself is refused by
    the engine; 0.01 is isotropic to a percent. 2e5 packets put 1.7e4
    events and more into each band and each sum 45 sigma and more from 0 on
    the restatement.

    The sign: Q > 0 in the equatorial band, Q < 0 in the meridian band - the
    sign the parallel camera's restatement gives left and right of a point
    source in its image."""
    model, field, centre = _pattern_model()
    e1 = centre - PATTERN_OBSERVER
    e1 /= np.sqrt(e1 @ e1)
    z = np.array([0., 0., 1.])
    pole = z - (z @ e1) * e1
    pole /= np.sqrt(pole @ pole)
    e2 = np.cross(pole, e1)
    tilted = np.cos(30. * DEG) * pole + np.sin(30. * DEG) * e2
    signs = []
    for p in (pole, tilted):
        cam = K.Camera(PATTERN_OBSERVER, 36, 18, 0.05,
                       frame=K.frame_of(p, e1), direct_light=False)
        assert np.allclose(cam.frame[0], e1, atol=1e-15)
        ref = K.Restatement(model, field, cam)
        ev = K.events(ref.trace(3, 0, PATTERN_PACKETS, 6), 6)
        l, b, _ = cam.angles(ev[:, :3])
        q, u = ev[:, 7] * ev[:, 4], ev[:, 7] * ev[:, 5]
        bands = {
            "equatorial": (np.abs(b) < 10. * DEG) & (np.abs(l) > 20. * DEG) &
                          (np.abs(l) < 60. * DEG),
            "meridian": (np.abs(l) < 10. * DEG) & (np.abs(b) > 20. * DEG) &
                        (np.abs(b) < 60. * DEG)}
        for name, sel in bands.items():
            sq, dq = _band(q[sel])
            su, _ = _band(u[sel])
            print(name, sel.sum(), "Q", sq, "+-", dq, "U", su)
            assert abs(sq) >= 5. * dq, (name, sq, dq)
            assert abs(su) < abs(sq), (name, su, sq)
            signs.append(np.sign(sq))
    assert signs[0] == -signs[1]
    assert signs[2:] == signs[:2]
    # the parallel camera: left and right of the source in its image (image
    # x = y cos phi - x sin phi, image y = the projected z axis, to which its
    # Q refers), single scatterings
    ev = K.events(ref.parallel_trace(3, 0, PATTERN_PACKETS, 8), 8)
    sp, cp, st, ct = (np.sin(model.phi), np.cos(model.phi),
                      np.sin(model.theta), np.cos(model.theta))

    def project(x):
        return (x[..., 1] * cp - x[..., 0] * sp,
                x[..., 2] * st - x[..., 1] * ct * sp - x[..., 0] * ct * cp)
    x0, y0 = project(centre)
    x, y = project(ev[:, :3])
    beside = (np.abs(y - y0) < 0.05) & (np.abs(x - x0) > 0.1) & \
        (np.abs(x - x0) < 0.35) & (ev[:, 4] != 0.)
    sq, dq = _band((ev[:, 7] * ev[:, 4])[beside])
    print("parallel camera, beside the source", beside.sum(), sq, "+-", dq)
    assert abs(sq) >= 5. * dq
    assert np.sign(sq) == signs[0] == 1.


# ------------------------------------------------------------ refusals --

BOX = ((-1., 0.5, 2.), (2.5, 3., 2.25))
INSIDE, OUTSIDE = (0.3, 2.1, 3.2), (5., 2.1, 3.2)


def _check(origin=INSIDE, nlon=8, nlat=4, r_min=0.2, **kw):
    from cmacionize_amd import engine as E
    E.check_sky_camera(BOX[0], BOX[1], origin, nlon, nlat, r_min, **kw)


def test_what_the_host_accepts():
    _check()
    _check(origin=OUTSIDE, r_min=0.)
    _check(lon_range=(1., 1. + 2. * np.pi))
    _check(lon_range=(10., 11.), lat_range=(-0.2, 0.1),
           frame=K.frame_of((1., 2., 3.), (0., 1., 0.)))
    _check(nlon=1 << 14, nlat=1 << 14)


@pytest.mark.parametrize("bad, message", [
    (dict(origin=(np.nan, 0., 0.)), "origin"),
    (dict(origin=(0., np.inf, 0.)), "origin"),
    (dict(frame=[[1., 0., 0.], [0., 1., 0.], [0., 1e-6, 1.]]), "orthonormal"),
    (dict(frame=2. * np.eye(3)), "orthonormal"),
    (dict(lon_range=(1., 1.)), "longitude"),
    (dict(lon_range=(0., np.inf)), "longitude"),
    (dict(lon_range=(0., 2. * np.pi + 1e-9)), "wider than 2 pi"),
    (dict(lon_range=(-np.pi, 3. * np.pi)), "wider than 2 pi"),
    (dict(lat_range=(-2., 1.)), "latitude"),
    (dict(lat_range=(0.5, 0.2)), "latitude"),
    (dict(nlon=0), "pixels"),
    (dict(nlat=-1), "pixels"),
    (dict(nlon=1 << 15, nlat=1 << 14), "pixels"),
    (dict(r_min=-0.1), "exclusion radius"),
    (dict(r_min=np.inf), "exclusion radius"),
    (dict(r_min=np.nan), "exclusion radius"),
    (dict(r_min=0.), "observer in the box"),
    # the closed box: an observer on a face
    (dict(origin=(1.5, 2.1, 3.2), r_min=0.), "observer in the box"),
    (dict(origin=(-1., 0.5, 2.), r_min=0.), "observer in the box"),
])
def test_what_the_host_refuses(bad, message):
    """6, first: every CMI_GPU_EINVAL of cmi_gpu_set_sky_camera, through
    cmi_gpu_check_sky_camera, the function that call runs its arguments
    through (the CMI_GPU_ESTATE cases need an engine:
    tests/test_gpu_scattered_sky.py)"""
    from cmacionize_amd import engine as E
    with pytest.raises(E.EngineError) as err:
        _check(**bad)
    assert message in str(err.value), str(err.value)
    assert "error %d" % K.EINVAL in str(err.value)


def test_library_exports_the_sky_camera():
    import ctypes as C
    from cmacionize_amd import engine
    lib = C.CDLL(engine.LIB_PATH)
    for name in ("cmi_gpu_set_sky_camera", "cmi_gpu_check_sky_camera",
                 "cmi_gpu_get_sky_camera_counters"):
        assert name in engine.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    for name in ("set_sky_camera", "get_sky_camera_counters",
                 "render_scattered_line_sky_map"):
        assert callable(getattr(engine.GpuEngine, name))
    assert engine.DUST_PROBE_SKY_PEEL == K.SKY_PEEL
    # the default pole is exactly z: the unrotated path
    assert np.array_equal(engine.sky_frame(), np.eye(3))
    assert np.allclose(engine.sky_frame((0., 1., 1.), (1., 0., 0.)),
                       K.frame_of((0., 1., 1.), (1., 0., 0.)), atol=1e-15)


# -------------------------------------------------------------- driver --

BLOCK_TEXT = ("EmissivityValues:\n  Halpha: true\n"
              "EmissionSkyMaps:\n  observer position: [0. m, 0. m, 0. m]\n"
              "  dust cross section per hydrogen: %s m^2\n")
DUST_KEYS = {"dust albedo": 0.54, "dust asymmetry": 0.44,
             "dust peak linear polarisation": 0.43}
ALL_KEYS = "  scattering: true\n  exclusion radius: 0.1 m\n" + "".join(
    "  %s: %r\n" % kv for kv in DUST_KEYS.items())


def _emission(tmp_path, text):
    params = tmp_path / "lines.param"
    params.write_text(text)
    r = subprocess.run([SL.CMI_GPU, "--emission", "--params", str(params),
                        "--file", str(tmp_path / "nowhere.hdf5")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    return r, str(params) + ".used-values"


def test_driver_parses_the_scattering_keys(tmp_path):
    """with every key the block is accepted (the run then fails on the
    snapshot, which does not exist); the keys and their defaults appear in
    the used-values"""
    r, used = _emission(tmp_path, BLOCK_TEXT % "2.e-27" + ALL_KEYS +
                        "  number of packets: 20000\n  random seed: 7\n"
                        "  direct light: false\n")
    assert r.returncode != 0 and "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    for word in ("scattering: true", "number of packets: 20000",
                 "random seed: 7", "dust albedo: 0.54", "dust asymmetry: 0.44",
                 "dust peak linear polarisation: 0.43", "exclusion radius",
                 "direct light: false"):
        assert word in used, (word, used)
    # defaults; without dust the three dust keys are not needed
    r, used = _emission(tmp_path, BLOCK_TEXT % "0." + "  scattering: true\n"
                        "  exclusion radius: 0.1 m\n")
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    assert "number of packets: 1000000" in used and "random seed: 42" in used
    assert "direct light: true" in used


@pytest.mark.parametrize("text, message", [
    (ALL_KEYS.replace("  exclusion radius: 0.1 m\n", ""),
     "exclusion radius is required"),
    (ALL_KEYS.replace("  dust albedo: 0.54\n", ""),
     "dust albedo is required"),
    (ALL_KEYS.replace("  dust asymmetry: 0.44\n", ""),
     "dust asymmetry is required"),
    (ALL_KEYS.replace("  dust peak linear polarisation: 0.43\n", ""),
     "dust peak linear polarisation is required"),
    (ALL_KEYS + "  number of packets: 0\n",
     "number of packets must be positive"),
    (ALL_KEYS.replace("0.54", "1.5"), "dust albedo must be in [0, 1]"),
    (ALL_KEYS.replace("0.44", "0."), "dust asymmetry must be non-zero"),
    (ALL_KEYS.replace("0.1 m", "-1. m"), "exclusion radius must be"),
    (ALL_KEYS + "  random seed: -1\n", "random seed"),
    (ALL_KEYS + "  longitude range: [-180. degrees, 270. degrees]\n",
     "longitude range must not be wider than 360 degrees"),
])
def test_driver_refuses_bad_scattering_values_first(tmp_path, text, message):
    """6, second: a bad key ends the run with its message before the
    snapshot is opened or a device touched"""
    r, used = _emission(tmp_path, BLOCK_TEXT % "2.e-27" + text)
    assert r.returncode != 0 and message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(used)


def test_driver_without_scattering_reads_none_of_the_new_keys(tmp_path):
    """6, third: a key that is read appears in the used-values with its
    default: none of the new ones does, with the switch absent or false; a
    range wider than 360 degrees stays allowed for the ray-traced map"""
    new = ("scattering", "number of packets", "random seed", "albedo",
           "asymmetry", "polarisation", "exclusion radius", "direct light")
    wide = "  longitude range: [-180. degrees, 270. degrees]\n"
    r, used = _emission(tmp_path, BLOCK_TEXT % "2.e-27" + wide)
    assert "Could not open" in r.stderr, r.stderr
    absent = open(used).read()
    assert "EmissionSkyMaps:" in absent
    for word in new:
        assert word not in absent, word
    r, used = _emission(tmp_path, BLOCK_TEXT % "2.e-27" + wide +
                        "  scattering: false\n")
    assert "Could not open" in r.stderr, r.stderr
    off = open(used).read()
    for word in new[1:]:
        assert word not in off, word
    # the switch itself is not counted as read either
    assert "scattering: value not used" in off
    assert [l for l in off.split("\n") if "scattering" not in l] == \
        absent.split("\n")
