"""The CPU restatement of the scattered-light line cubes
(tests/support/scattered_cube_reference.c) on its own, and the driver's new
key - no GPU. The restatement is held to what follows from the contract
(include/cmi_gpu.h, "scattered-light line cubes"): identities 1 to 4, the
albedo-0 identity with the ray-traced cubes' restatements (line_cube_lib,
sky_cube_lib) per pixel and channel, a delta line on and off a channel edge,
and the Galilean identity for packets that scatter several times. The GPU
tests (test_gpu_scattered_cube.py) then hold the device to the restatement."""
import os
import subprocess

import numpy as np
import pytest

import line_cube_lib as LC
import scattered_cube_lib as Q
import scattered_line_lib as SL
import scattered_sky_lib as SS
import sky_cube_lib as SC

WIDE = 1.0e6  # m s^-1: +- WIDE covers u +- 6 b of every event below
N = 20000
SEED = 5


def _scene(albedo, point, sigma=None):
    """identity_model's 10 x 12 x 9 box with 16 x 16 pixels; for the point
    camera identity_scene's observer with a 16 x 16 map"""
    box, model, field = SL.identity_model(albedo)
    if sigma is not None:
        model.sigma = sigma
    cam = None
    if point:
        r_min = float((model.sides / model.ncell).max())
        cam = SS.Camera(SS.IDENTITY_OBSERVER, 16, 16, r_min)
    return box, model, field, cam


def _moving(model, nchan, vmin, vmax, **kw):
    """the trace scene's shear, rotation, widths and turbulence"""
    v, _, _ = Q.trace_velocity(model)
    return Q.Cube(nchan, vmin, vmax, Q.trace_widths(model),
                  Q.TRACE_SIGMA_TURB, v, **kw)


def _close(a, b, scale, rtol=1e-12, atol=1e-14):
    return np.allclose(a, b, rtol=rtol, atol=atol * np.abs(scale).max())


@pytest.mark.parametrize("point", [False, True])
def test_one_covering_channel_is_the_image(point):
    """1. f_0 = 1 exactly: the same addends in the same order"""
    box, model, field, cam = _scene(0.6, point)
    ref = Q.Restatement(model, field, _moving(model, 1, -WIDE, WIDE), cam)
    image, cube, c = ref.shoot(SEED, 0, N)
    assert c[1] > N / 2 and c[2] == 0 and c[5] > N
    assert np.abs(image[1]).max() > 0. and np.abs(image[2]).max() > 0.
    assert np.array_equal(cube[:, 0], image)


@pytest.mark.parametrize("point", [False, True])
@pytest.mark.parametrize("nchan", [5, 8, 9, 19])
def test_covering_channels_sum_to_the_image(point, nchan):
    """2. up to rounding: a channel's share is a difference of two erf
    values of magnitude <= 1, nchan of them telescope to 1 with an error of
    a few nchan eps"""
    box, model, field, cam = _scene(0.6, point)
    ref = Q.Restatement(model, field, _moving(model, nchan, -WIDE, WIDE), cam)
    image, cube, c = ref.shoot(SEED, 0, N)
    assert _close(cube.sum(axis=1), image, image[0])
    # and the light is not all in one channel: a narrower axis resolves it
    ref = Q.Restatement(model, field, _moving(model, nchan, -4.0e4, 4.0e4),
                        cam)
    image2, cube2, _ = ref.shoot(SEED, 0, N)
    assert _close(image2, image, image[0])  # (the threads' order differs)
    assert np.count_nonzero(cube2[0].sum(axis=(1, 2))) == nchan
    assert np.all(cube2[0].sum(axis=0) <= image[0] * (1. + 1e-12))


def test_galilean_identity_parallel():
    """3. adding V to every cell velocity shifts every u by -dot3(V, d): the
    cube on the axis shifted by as much is the same up to rounding. u and the
    edges are of order 3e4 and rounded to 4e-12; over b of 1e4 that moves an
    erf argument by 1e-15 and a share by as much, absolutely: rtol 1e-9 of
    the pixel's image value covers it a million times over and is still far
    below one channel's share."""
    box, model, field, cam = _scene(0.6, False)
    nchan, vmin, vmax = 9, -3.0e4, 3.0e4
    V = np.array([7.0e3, -1.1e4, 4.0e3])
    d = np.array([np.sin(model.theta) * np.cos(model.phi),
                  np.sin(model.theta) * np.sin(model.phi),
                  np.cos(model.theta)])
    shift = -float(V @ d)
    a = _moving(model, nchan, vmin, vmax)
    ref = Q.Restatement(model, field, a, cam)
    image, cube, _ = ref.shoot(SEED, 0, N)
    v, _, _ = Q.trace_velocity(model)
    b = Q.Cube(nchan, vmin + shift, vmax + shift, a.widths, a.sigma_turb,
               v + V)
    image_b, cube_b, _ = Q.Restatement(model, field, b, cam).shoot(SEED, 0, N)
    assert _close(image_b, image, image[0])
    assert np.allclose(cube_b, cube, rtol=0.,
                       atol=1e-9 * np.abs(image[:, None]) + 1e-300)
    # not trivially: on the unshifted axis the boosted cube differs
    c = Q.Cube(nchan, vmin, vmax, a.widths, a.sigma_turb, v + V)
    cube_c = Q.Restatement(model, field, c, cam).shoot(SEED, 0, N)[1]
    assert not np.allclose(cube_c, cube, rtol=1e-3, atol=0.)


def test_galilean_identity_point():
    """3. for the point camera the observer is boosted as well and nothing
    changes (the same bound)"""
    box, model, field, cam = _scene(0.6, True)
    nchan, vmin, vmax = 9, -3.0e4, 3.0e4
    V = np.array([7.0e3, -1.1e4, 4.0e3])
    vo = np.array([1.0e3, 2.0e3, -3.0e3])
    v, _, _ = Q.trace_velocity(model)
    a = _moving(model, nchan, vmin, vmax, observer_velocity=vo)
    image, cube, _ = Q.Restatement(model, field, a, cam).shoot(SEED, 0, N)
    b = Q.Cube(nchan, vmin, vmax, a.widths, a.sigma_turb, v + V, vo + V)
    image_b, cube_b, _ = Q.Restatement(model, field, b, cam).shoot(SEED, 0, N)
    assert _close(image_b, image, image[0])
    assert np.allclose(cube_b, cube, rtol=0.,
                       atol=1e-9 * np.abs(image[:, None]) + 1e-300)
    c = Q.Cube(nchan, vmin, vmax, a.widths, a.sigma_turb, v + V, vo)
    cube_c = Q.Restatement(model, field, c, cam).shoot(SEED, 0, N)[1]
    assert not np.allclose(cube_c, cube, rtol=1e-3, atol=0.)


def test_galilean_identity_after_several_scatterings():
    """3. with albedo 0.9 and optical depths of 3 to 10 across the box the
    packets scatter more than twice on average: the sum over scatterings
    telescopes"""
    box, model, field, cam = _scene(0.9, False, sigma=0.25)
    nchan, vmin, vmax = 9, -3.0e4, 3.0e4
    V = np.array([-5.0e3, 9.0e3, 6.0e3])
    d = np.array([np.sin(model.theta) * np.cos(model.phi),
                  np.sin(model.theta) * np.sin(model.phi),
                  np.cos(model.theta)])
    shift = -float(V @ d)
    v, _, _ = Q.trace_velocity(model)
    a = _moving(model, nchan, vmin, vmax)
    image, cube, c = Q.Restatement(model, field, a).shoot(SEED, 0, N)
    assert c[1] / N > 2., c[1] / N
    b = Q.Cube(nchan, vmin + shift, vmax + shift, a.widths, a.sigma_turb,
               v + V)
    image_b, cube_b, _ = Q.Restatement(model, field, b).shoot(SEED, 0, N)
    assert _close(image_b, image, image[0])
    assert np.allclose(cube_b, cube, rtol=0.,
                       atol=1e-9 * np.abs(image[:, None]) + 1e-300)


@pytest.mark.parametrize("point", [False, True])
def test_gas_at_rest_with_one_width_gives_the_image_times_a_constant(point):
    """4. all cells at rest, sigma_t = 0, one width: f_c(0, b) per channel"""
    box, model, field, cam = _scene(0.6, point)
    nchan, b = 8, 9.0e3
    q = Q.Cube(nchan, -2.0e4, 2.4e4, np.full(model.n, b))
    ref = Q.Restatement(model, field, q, cam)
    image, cube, _ = ref.shoot(SEED, 0, N)
    f = ref.shares(0., b)
    assert np.allclose(f, LC.fractions(nchan, -2.0e4, 2.4e4, 0., b),
                       rtol=1e-12, atol=1e-17)
    assert f.min() > 0.
    assert _close(cube, image[:, None] * f[None, :, None, None], image[0])


def _judge(mc, squares, hits, rt, scale):
    """test_scattered_line_host.py's judgement per element: elements with at
    least 100 contributions, at least three quarters of those the ray tracer
    lights above 1e-6 of its peak; z <= 5, and z of order one"""
    lit = rt > 1e-6 * rt.max()
    judged = lit & (hits >= 100)
    print("lit", lit.sum(), "judged", judged.sum())
    assert lit.sum() > 100 and judged.sum() >= 0.75 * lit.sum()
    z = np.abs(mc * scale - rt)[judged] / (np.sqrt(squares) * scale)[judged]
    print("worst", z.max(), "rms", np.sqrt(np.mean(z ** 2)))
    assert z.max() <= 5.
    assert 0.5 < np.sqrt(np.mean(z ** 2)) < 1.5


def test_albedo_0_is_the_ray_traced_cube():
    """5. only the direct light reaches the cube, and its expectation per
    pixel and channel is the ray-traced cube with extinction n sigma
    (line_cube_reference.c with 8 x 8 samples per pixel), in the unit of the
    scattered images' scaling. The variance is that of the restatement's own
    addends."""
    box, model, field, _ = _scene(0., False)
    nchan, vmin, vmax = 8, -3.2e4, 3.2e4
    v, _, _ = Q.trace_velocity(model)
    widths = Q.trace_widths(model)
    q = Q.Cube(nchan, vmin, vmax, widths, 0., v)
    ref = Q.Restatement(model, field, q)
    n = SL.IDENTITY_PACKETS
    image, cube, c, squares, hits = ref.shoot(SL.IDENTITY_SEED, 0, n, True)
    assert c[1] > 0 and not cube[1].any() and not cube[2].any()
    total = np.zeros(1)
    Q.lib().slref_get_tables(Q._p(total), None, None)
    scale = float(total[0]) / (n * model.pixel_area)
    rt = LC.render(box, field, widths, model.theta, model.phi, model.nx,
                   model.ny, model.img_anchor, model.img_sides, nchan, vmin,
                   vmax, 8, extinction=model.density * model.sigma,
                   velocity=q.velocity)[0]
    _judge(cube[0], squares, hits, rt, scale)


def test_albedo_0_is_the_ray_traced_sky_cube():
    """5. for the observer inside (scattered_sky_lib.identity_scene, whose
    field is dark within r_min of the observer) with a velocity of its own:
    sky_cube_reference.c on 8 x 8 directions of equal solid angle per
    pixel"""
    box, model, field, mask, cam = SS.identity_scene()
    nchan, vmin, vmax = 8, -3.2e4, 3.2e4
    v, _, _ = Q.trace_velocity(model)
    widths = Q.trace_widths(model)
    vo = np.array([4.0e3, -6.0e3, 2.0e3])
    q = Q.Cube(nchan, vmin, vmax, widths, 0., v, vo)
    ref = Q.Restatement(model, field, q, cam)
    n = SS.IDENTITY_PACKETS
    image, cube, c, squares, hits = ref.shoot(SS.IDENTITY_SEED, 0, n, True)
    assert c[2] == 0 and c[4] == 0
    total = np.zeros(1)
    Q.lib().slref_get_tables(Q._p(total), None, None)
    scale = float(total[0]) / n / cam.solid_angles()
    d = SS.subray_directions(cam, 8)
    rt = SC.render(box, field, widths, cam.origin, d.reshape(-1, 3), nchan,
                   vmin, vmax, extinction=model.density * model.sigma,
                   velocity=q.velocity, observer_velocity=vo)[0]
    rt = rt.reshape(nchan, cam.nlon, cam.nlat, -1).mean(axis=3)
    _judge(cube[0], squares, hits, rt, scale[None])


def _delta_line(vx):
    """one emitting cell of the identity box, b = 0, every cell moving with
    (vx, 0, 0), albedo 0: every direct event has u = -(vx d_x)"""
    box, model, field, _ = _scene(0., False)
    one = np.zeros(model.n)
    one[517] = 1.
    v = np.zeros((model.n, 3))
    v[:, 0] = vx
    # 5 channels of 1024 m/s from -5120: the edge e_2 is -3072 exactly
    q = Q.Cube(5, -5120., 0., np.zeros(model.n), 0., v)
    return Q.Restatement(model, one, q)


def test_delta_line_on_and_off_a_channel_edge():
    """b = 0 is the step function with the lower edge inclusive: a line at u
    == e_c belongs to channel c, one ulp below it to channel c - 1"""
    box, model, field, _ = _scene(0., False)
    dx = np.sin(model.theta) * np.cos(model.phi)
    vx = 3072. / dx
    on = None
    for _ in range(64):  # the neighbours of 3072 / d_x, either way
        for cand in (vx, -vx + 2. * 3072. / dx):
            u = _delta_line(cand).trace(SEED, 0, 1, 4)[0, 4 + 8]
            if u == -3072.:
                on = cand
        if on is not None:
            break
        vx = np.nextafter(vx, np.inf)
    assert on is not None, "no velocity puts u on the edge"
    for vx, channel in ((on, 2), (on * (1. + 1e-12), 1),
                        (on * (1. - 1e-12), 2)):
        ref = _delta_line(vx)
        row = ref.trace(SEED, 0, 1, 4)[0, 4:14]
        assert row[9] == 0.  # b
        assert (row[8] == -3072.) == (vx == on)
        image, cube, c = ref.shoot(SEED, 0, 2000)
        assert image[0].sum() > 0.
        lit = np.flatnonzero(cube[0].sum(axis=(1, 2)))
        assert list(lit) == [channel], (vx, lit)
        assert np.array_equal(cube[0, channel], image[0])


@pytest.mark.parametrize("point", [False, True])
def test_trace_seed_has_no_position_on_a_cell_wall(point):
    """the GPU's trace test may leave out rows within 1e-9 cell sides of a
    cell wall (the scattering cell could differ); its seed has none"""
    box, model, field, cam = _scene(0.6, point)
    ref = Q.Restatement(model, field, _moving(model, 9, -4.0e4, 4.0e4), cam)
    cap = 64
    tr = ref.trace(Q.TRACE_SEED, 0, 256, cap)
    assert tr[:, 0].max() < cap and tr[:, 1].max() >= 3
    rows = Q.events(tr, cap)
    assert len(rows) > 400
    assert not Q.near_wall(model, rows[:, 0:3]).any()


# -------------------------------------------------------------- driver --

GOLDEN = os.path.join(SL.HERE, "golden", "multi_view")
ONE_VIEW = open(os.path.join(GOLDEN, "one_view_lines.param")).read()
IMAGES, SKY = ONE_VIEW.split("EmissionSkyMaps:\n")
SKY = "EmissionSkyMaps:\n" + SKY
CHANNELS = ("  velocity channels: 8\n  velocity minimum: -40. km s^-1\n"
            "  velocity maximum: 40. km s^-1\n")
KEY = "  scattered cubes: %s\n"


def _emission(tmp_path, text, dry_run=True):
    params = tmp_path / "lines.param"
    params.write_text(text)
    used = str(params) + ".used-values"
    if os.path.exists(used):
        os.remove(used)
    cmd = [SL.CMI_GPU, "--emission", "--params", str(params), "--file",
           str(tmp_path / "nowhere.hdf5")]
    if dry_run:
        cmd.insert(2, "--dry-run")
    r = subprocess.run(cmd, capture_output=True, text=True,
                       cwd=str(tmp_path))
    return r, used


@pytest.mark.parametrize("text, message", [
    (IMAGES + KEY % "true" + SKY,
     "EmissionImages:scattered cubes needs velocity channels"),
    (IMAGES.replace("scattering: true", "scattering: false") + CHANNELS +
     KEY % "true" + SKY,
     "EmissionImages:scattered cubes needs scattering: true"),
    (IMAGES.replace("  scattering: true\n", "") + CHANNELS + KEY % "true" +
     SKY, "EmissionImages:scattered cubes needs scattering: true"),
    (IMAGES + SKY + KEY % "true",
     "EmissionSkyMaps:scattered cubes needs velocity channels"),
    (IMAGES + SKY.replace("scattering: true", "scattering: false") +
     CHANNELS + KEY % "true",
     "EmissionSkyMaps:scattered cubes needs scattering: true"),
])
def test_driver_refuses(tmp_path, text, message):
    r, used = _emission(tmp_path, text)
    assert r.returncode != 0 and message in r.stderr, r.stderr
    assert "Could not open" not in r.stderr
    assert not os.path.exists(used)


def test_driver_accepts_the_key_and_lists_it(tmp_path):
    text = IMAGES + CHANNELS + KEY % "true" + SKY + CHANNELS + KEY % "true"
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    used = open(used).read()
    assert used.count("scattered cubes: true") == 2


def test_driver_without_the_key_reads_nothing_new(tmp_path):
    """with the key absent the used-values are what they were (the golden
    file of the block without cubes, and the same text with cubes); with the
    key false it is listed as not used and nothing else changes"""
    r, used = _emission(tmp_path, ONE_VIEW, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    assert open(used).read() == \
        open(os.path.join(GOLDEN, "one_view_lines.param.usedvalues")).read()
    text = IMAGES + CHANNELS + SKY + CHANNELS
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    absent = open(used).read()
    assert "scattered cubes" not in absent
    text = IMAGES + CHANNELS + KEY % "false" + SKY + CHANNELS + KEY % "false"
    r, used = _emission(tmp_path, text, dry_run=False)
    assert "Could not open" in r.stderr, r.stderr
    off = open(used).read()
    assert off.count("scattered cubes: value not used") == 2
    assert [l for l in off.split("\n") if "scattered cubes" not in l] == \
        absent.split("\n")
