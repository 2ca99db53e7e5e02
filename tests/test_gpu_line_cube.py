"""Spectral line cubes on the device (cmi_gpu_render_field_cube,
cmi_gpu_render_line_cube, cmi_gpu_set_cell_velocities) against
the identities of the contract, against the CPU restatement
(tests/support/line_cube_reference.c, checked on its own in
test_line_cube_host.py) and against themselves."""
import ctypes as C

import numpy as np
import pytest

import line_cube_lib as Q
import line_image_lib as L
from test_gpu_emissivity import random_state
from test_gpu_physics import lexington_engine

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BOX, NX, NY, VIEWS = Q.BOX, Q.NX, Q.NY, Q.VIEWS
SUPERSAMPLE = (1, 2, 1, 2, 1, 2)   # per view
CB = Q.channel_block()
EINVAL, ESTATE = 1, 3  # include/cmi_gpu.h
# The error of the device's erf in ulps. The ROCm documentation installed
# with the toolchain states no bound for erf, so it was measured once on an
# MI355X through render_field_cube on single-cell rays, at 10^6 points of
# [-6, 6] against glibc's erf: at most 2 ulps of erf (1 eps of E; 1.6 % of the
# points differ at all), doubled as the margin.
U_DEV = 4.
U_CPU = 1.   # glibc's erf


def plain_engine(box):
    from cmacionize_amd import GpuEngine
    return GpuEngine(tuple(int(n) for n in box.ncell), tuple(box.anchor),
                     tuple(box.sides), (0, 0, 0), device=0)


@pytest.fixture(scope="module")
def eng():
    engine = plain_engine(BOX)
    yield engine
    engine.close()


def random_cells(seed):
    """fields 10^U(-2, 1) with some dark cells, widths over a factor of 30
    with some cold cells, |v| <= 32 b per component's norm, extinction with
    optical depths per cell around 0.1 and some cells without dust"""
    rng = np.random.default_rng(seed)
    fields = 10. ** rng.uniform(-2., 1., (2, BOX.n))
    fields[rng.uniform(size=(2, BOX.n)) < 0.1] = 0.
    widths = 10. ** rng.uniform(0., np.log10(30.), (2, BOX.n))
    widths[rng.uniform(size=(2, BOX.n)) < 0.1] = 0.
    direction = rng.normal(size=(3, BOX.n))
    direction /= np.linalg.norm(direction, axis=0)
    speed = 32. * np.maximum(widths[0], 1.) * rng.uniform(0., 1., BOX.n)
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n)
    k[rng.uniform(size=BOX.n) < 0.1] = 0.
    return fields, widths, direction * speed, k


def test_identity_1_one_wide_channel_is_the_image(eng):
    """Case 1: nchan = 1 over a range that covers u +- 6 b of every cell: f_0
    = 0.5 * (1 - -1) = 1 and the cube is render_field_images, bit for bit, in
    all six views at s = 1 and 2, without and with dust: the cube kernel
    marches the image kernel's cells."""
    fields, widths, vel, k = random_cells(41)
    reach = np.abs(vel).sum(axis=0).max() + 6. * widths.max()
    for theta, phi in VIEWS:
        anchor, sides = Q.image_rectangle(BOX, theta, phi)
        for s in (1, 2):
            for ext in (None, k):
                image = eng.render_field_images(fields, theta, phi, NX, NY,
                                                anchor, sides, s,
                                                extinction=ext)
                cube = eng.render_field_cube(
                    fields, widths, theta, phi, NX, NY, anchor, sides, 1,
                    -reach, reach, s, extinction=ext, velocity=vel)
                assert cube.shape == (2, 1, NX, NY)
                assert (image > 0.).sum() > 0.3 * image.size
                assert (image == 0.).sum() > 20
                assert np.array_equal(cube[:, 0], image), (theta, phi, s)


@pytest.mark.parametrize("nchan", sorted({1, 5, CB, CB + 1, 2 * CB + 3}))
def test_parity_with_the_restatement(eng, nchan):
    """Case 2: per pixel and channel |gpu - cpu| <= eps (8 steps I_c + (U_dev
    + U_cpu + 4 max((|u| + |e|) / b)) I_tot): 8 eps per step for exp and
    expm1 as in the line images, the two erfs' errors, and the rounding of e
    - u and of the division by b carried through erf (slope <= 2 / sqrt(pi)),
    each weighted with what a step can add, whose sum over the ray is at most
    the integrated image I_tot. The range cuts through the emission on its
    lower side. No pixel is left out."""
    fields, widths, vel, k = random_cells(43)
    vmin, vmax = -150., 1100.
    edges = Q.edges(nchan, vmin, vmax)
    worst = 0.
    for (theta, phi), s in zip(VIEWS, SUPERSAMPLE):
        anchor, sides = Q.image_rectangle(BOX, theta, phi)
        n, _, _ = L.axes(theta, phi)
        u = -((vel[0] * n[0] + vel[1] * n[1]) + vel[2] * n[2])
        warm = widths > 0.
        reach = np.broadcast_to(np.abs(u) + np.abs(edges).max(),
                                widths.shape)
        slope = (reach[warm] / widths[warm]).max()
        steps = Q.longest_ray(BOX, theta, phi, NX, NY, anchor, sides, s)
        for ext in (None, k):
            want = Q.render(BOX, fields, widths, theta, phi, NX, NY, anchor,
                            sides, nchan, vmin, vmax, s, extinction=ext,
                            velocity=vel)
            total = L.render(BOX, fields, theta, phi, NX, NY, anchor, sides,
                             s, extinction=ext)
            got = eng.render_field_cube(fields, widths, theta, phi, NX, NY,
                                        anchor, sides, nchan, vmin, vmax, s,
                                        extinction=ext, velocity=vel)
            assert got.shape == want.shape == (2, nchan, NX, NY)
            assert not np.isnan(got).any()
            # the range cuts: part of the emission is outside it
            assert 0.2 * total.sum() < want.sum() < 0.98 * total.sum()
            bound = EPS * (8. * steps * want +
                           (U_DEV + U_CPU + 4. * slope) * total[:, None])
            diff = np.abs(got - want)
            dark = bound == 0.
            assert not got[dark].any() and not want[dark].any()
            ratio = (diff[~dark] / bound[~dark]).max()
            worst = max(worst, ratio)
            print("nchan", nchan, "view", theta, phi, "s", s, "dust",
                  ext is not None, "steps", steps, "slope", slope,
                  "worst |gpu - cpu| / bound", ratio)
            assert (diff <= bound).all()
    print("nchan", nchan, "worst ratio of difference to bound", worst)


@pytest.mark.parametrize("s, nx", [(8, 2048 + 50), (1, 131072 + 50)])
def test_more_pixel_rows_than_one_launch_takes(eng, s, nx):
    """Case 2, the chunks of pixel rows: a launch takes 2^22 / CB sample rays,
    with ny = 4 that is 2048 pixel rows at s = 8 and 131072 at s = 1, and a
    second launch marches the last 50, for nchan = CB + 1 in two channel
    blocks each - through the sample buffer and one reduction per field at
    s = 8, straight into the cube at its row offset at s = 1. Two fields with
    velocities, no extinction, the bound of Case 2, on the middle of the
    oblique view's rectangle so that the last chunk's pixels are lit."""
    ny, nchan = 4, CB + 1
    rows = ((1 << 22) // CB) // (ny * s * s)
    assert nx == rows + 50
    fields, widths, vel, _ = random_cells(47)
    vmin, vmax = -150., 150.   # every channel has emission in the last rows
    edges = Q.edges(nchan, vmin, vmax)
    theta, phi = 0.7, 0.3
    anchor, sides = L.bounding_rectangle(BOX, theta, phi)
    anchor, sides = anchor + 0.25 * sides, 0.5 * sides
    n, _, _ = L.axes(theta, phi)
    u = -((vel[0] * n[0] + vel[1] * n[1]) + vel[2] * n[2])
    warm = widths > 0.
    reach = np.broadcast_to(np.abs(u) + np.abs(edges).max(), widths.shape)
    slope = (reach[warm] / widths[warm]).max()
    steps = Q.longest_ray(BOX, theta, phi, nx, ny, anchor, sides, s)
    want = Q.render(BOX, fields, widths, theta, phi, nx, ny, anchor, sides,
                    nchan, vmin, vmax, s, velocity=vel)
    total = L.render(BOX, fields, theta, phi, nx, ny, anchor, sides, s)
    got = eng.render_field_cube(fields, widths, theta, phi, nx, ny, anchor,
                                sides, nchan, vmin, vmax, s, velocity=vel)
    assert got.shape == want.shape == (2, nchan, nx, ny)
    assert not np.isnan(got).any()
    assert (total > 0.).all()
    # the last chunk, and in it the second channel block, are lit
    assert (want[:, CB:, rows:] > 0.).any()
    assert (got[:, :, rows:] > 0.).any() and (got[:, CB:, rows:] > 0.).any()
    bound = EPS * (8. * steps * want +
                   (U_DEV + U_CPU + 4. * slope) * total[:, None])
    diff = np.abs(got - want)
    print("s", s, "nx", nx, "steps", steps, "slope", slope,
          "worst |gpu - cpu| / bound", (diff / bound).max())
    assert (diff <= bound).all()


def test_identity_2_and_the_sign_of_the_velocity(eng):
    """Case 3: theta = 0 (n = (0, 0, 1) exactly), velocities along n and
    edges in multiples of 2^-3: D = 40 added to every u and to the range
    leaves every e - u, hence the cube, as it is. One emitting cold cell
    moving towards the observer with V lights the channel that holds -V."""
    rng = np.random.default_rng(47)
    fields = 10. ** rng.uniform(-2., 1., (1, BOX.n))
    widths = 10. ** rng.uniform(0., 1., (1, BOX.n))
    vel = np.zeros((3, BOX.n))
    vel[2] = rng.integers(-80, 81, BOX.n) / 8.
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n)
    anchor, sides = Q.image_rectangle(BOX, 0., 0.)
    D, nchan = 40., 2 * CB + 3
    lo, hi = -9.5, -9.5 + nchan * 0.875
    a = eng.render_field_cube(fields, widths, 0., 0., NX, NY, anchor, sides,
                              nchan, lo, hi, 2, extinction=k, velocity=vel)
    shifted = vel.copy()
    shifted[2] -= D   # u = -v_z grows by D
    b = eng.render_field_cube(fields, widths, 0., 0., NX, NY, anchor, sides,
                              nchan, lo + D, hi + D, 2, extinction=k,
                              velocity=shifted)
    assert (a > 0.).sum() > 0.3 * a.size
    assert np.array_equal(a, b)

    V = 3.3
    cell = (5 * BOX.ncell[1] + 4) * BOX.ncell[2] + 3
    j = np.zeros(BOX.n)
    j[cell] = 1.
    vel = np.zeros((3, BOX.n))
    vel[2, cell] = V   # along n: towards the observer
    cube = eng.render_field_cube(j, np.zeros(BOX.n), 0., 0., NX, NY, anchor,
                                 sides, 10, -5., 5., velocity=vel)[0]
    image = eng.render_field_images(j, 0., 0., NX, NY, anchor, sides)[0]
    assert image.max() > 0.
    assert np.array_equal(cube[1], image)   # [-4, -3) holds -3.3
    assert not np.delete(cube, 1, axis=0).any()


def test_identity_3_the_channels_sum_to_the_image(eng):
    """Case 4: with a range that covers u +- 6 b of every cell the sum over
    channels is the image within (nchan + 8 steps) eps relative"""
    fields, widths, vel, k = random_cells(53)
    reach = np.abs(vel).sum(axis=0).max() + 6. * widths.max()
    nchan = 2 * CB + 3
    for (theta, phi), s in zip(VIEWS, SUPERSAMPLE):
        anchor, sides = Q.image_rectangle(BOX, theta, phi)
        steps = Q.longest_ray(BOX, theta, phi, NX, NY, anchor, sides, s)
        for ext in (None, k):
            image = eng.render_field_images(fields, theta, phi, NX, NY,
                                            anchor, sides, s, extinction=ext)
            cube = eng.render_field_cube(fields, widths, theta, phi, NX, NY,
                                         anchor, sides, nchan, -reach, reach,
                                         s, extinction=ext, velocity=vel)
            total = cube.sum(axis=1)
            lit = image > 0.
            assert not total[~lit].any()
            err = np.abs(total - image)[lit] / image[lit]
            print("view", theta, phi, "s", s, "dust", ext is not None,
                  "worst", err.max(), "allowed", (nchan + 8 * steps) * EPS)
            assert err.max() <= (nchan + 8 * steps) * EPS
            # a narrower range gives less, never more
            part = eng.render_field_cube(fields, widths, theta, phi, NX, NY,
                                         anchor, sides, nchan, 0.02 * reach,
                                         0.3 * reach, s, extinction=ext,
                                         velocity=vel).sum(axis=1)
            assert (part <= image * (1. + (nchan + 8 * steps) * EPS)).all()
            # (the directions are isotropic, so u is as often negative as
            # positive: a range on one side of 0 holds about half at most)
            assert part.sum() < 0.75 * image.sum()


def test_line_cube_end_to_end(oracle):
    """Case 5: the random lexington state of the line-image test with a
    radial expansion: H alpha and [O III] 5007 in one call against the
    restatement fed with the oracle's emissivities and with widths from the
    table of atomic weights in numpy, within the line-image test's 2e-10 (of
    the pixel's integrated brightness, which is what an emissivity's own
    difference scales with). With sigma_turb = 0 the [O III] line is narrower
    than H alpha by sqrt(15.9994 / 1.00794)."""
    import oracle_lib as o
    from cmacionize_amd import engine as E
    ncell = 12
    sim = oracle.lexington_simulation(ncell)
    density, temperature, x = random_state(ncell, 7)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    box = L.Box((-5. * o.PC,) * 3, (10. * o.PC,) * 3, (ncell,) * 3)
    n = ncell ** 3
    names = ["HAlpha", "OIII_5007"]
    ref = np.array([oracle.emissivities(sim.model, density[c], temperature[c],
                                        x[:, c]) for c in range(n)]).T
    ref = ref[[E.EMISSION_LINES.index(name) for name in names]]
    # v = v0 r / r0 about the centre of the box
    idx = np.stack(np.meshgrid(*[np.arange(ncell)] * 3, indexing="ij"))
    r = (box.anchor[:, None] + (idx.reshape(3, n) + 0.5) *
         box.cellside[:, None])
    vel = 15.e3 * r / (5. * o.PC)
    eng.set_cell_velocities(vel)
    k_B, m_u = 1.38064852e-23, 1.660539040e-27
    sigma_dust = 2.e-27
    nchan, vmin, vmax = 96, -48.e3, 48.e3
    for (theta, phi), s, turb in (((0.7, 0.3), 1, 0.), ((2.1, 4.0), 2, 4.e3)):
        widths = np.array([np.sqrt(2. * (k_B * temperature /
                                         (E.LINE_ATOMIC_WEIGHTS[name] * m_u) +
                                         turb * turb)) for name in names])
        anchor, sides = L.bounding_rectangle(box, theta, phi)
        nx, ny = 23, 17
        for sigma in (0., sigma_dust):
            ext = density * sigma if sigma else None
            got = eng.render_line_cube(names, theta, phi, nx, ny, anchor,
                                       sides, nchan, vmin, vmax, s, sigma,
                                       turb)
            assert list(got) == names
            want = Q.render(box, ref, widths, theta, phi, nx, ny, anchor,
                            sides, nchan, vmin, vmax, s, extinction=ext,
                            velocity=vel)
            total = L.render(box, ref, theta, phi, nx, ny, anchor, sides, s,
                             extinction=ext)
            for l, name in enumerate(names):
                assert got[name].shape == (nchan, nx, ny)
                lit = total[l] > 0.
                assert lit.sum() > 0.3 * nx * ny
                assert not got[name][:, ~lit].any()
                err = (np.abs(got[name] - want[l])[:, lit] /
                       total[l][lit]).max()
                print(name, "view", theta, phi, "dust", sigma, "turb", turb,
                      "worst / I_tot", err)
                assert err < 2.e-10, (name, sigma, err)
    # the widths of the two lines: the same cells at rest at one temperature,
    # so that the thermal width is all there is; channels of 200 m s^-1
    # against sigma = 2.0 km s^-1 of [O III] at 8000 K
    eng.upload_cells(density, np.full(n, 8000.), x)
    eng.set_cell_velocities(None)
    anchor, sides = L.bounding_rectangle(box, 0.7, 0.3)
    still = eng.render_line_cube(names, 0.7, 0.3, 23, 17, anchor, sides, 480,
                                 vmin, vmax)
    centres = E.cube_channel_centres(480, vmin, vmax)
    m0_h, _, disp_h = E.cube_moments(still["HAlpha"], centres)
    m0_o, _, disp_o = E.cube_moments(still["OIII_5007"], centres)
    pixel = np.unravel_index(np.argmax(m0_o), m0_o.shape)
    assert m0_h[pixel] > 0. and m0_o[pixel] > 0.
    ratio = disp_h[pixel] / disp_o[pixel]
    expect = np.sqrt(15.9994 / 1.00794)
    print("dispersions", disp_h[pixel], disp_o[pixel], "ratio", ratio,
          "expected about", expect)
    assert abs(ratio / expect - 1.) < 0.05
    eng.close()


def test_repeats_velocities_and_bad_arguments(eng):
    """Case 6: two identical calls give identical bits; None velocities are
    zero velocities; every refusal of include/cmi_gpu.h, with the engine
    usable afterwards."""
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    fields, widths, vel, k = random_cells(59)
    theta, phi = VIEWS[3]
    anchor, sides = Q.image_rectangle(BOX, theta, phi)
    args = (theta, phi, NX, NY, anchor, sides, CB + 3, -300., 700., 2)
    a = eng.render_field_cube(fields, widths, *args, extinction=k,
                              velocity=vel)
    b = eng.render_field_cube(fields, widths, *args, extinction=k,
                              velocity=vel)
    assert a.any() and np.array_equal(a, b)
    rest = eng.render_field_cube(fields, widths, *args, extinction=k)
    zero = eng.render_field_cube(fields, widths, *args, extinction=k,
                                 velocity=np.zeros((3, BOX.n)))
    assert np.array_equal(rest, zero) and not np.array_equal(rest, a)
    for bad in (-1., np.inf, np.nan):
        w = widths.copy()
        w[1, 17] = bad
        with pytest.raises(E.EngineError, match="width"):
            eng.render_field_cube(fields, w, *args)
    for bad in (np.inf, np.nan):
        v = vel.copy()
        v[2, 5] = bad
        with pytest.raises(E.EngineError, match="not finite"):
            eng.render_field_cube(fields, widths, *args, velocity=v)
    for nchan, lo, hi in ((0, -1., 1.), (-2, -1., 1.), (4, 1., 1.),
                          (4, 2., 1.), (4, -np.inf, 1.), (4, 0., np.nan),
                          (4, -1.e308, 1.e308),
                          ((1 << 28) // (NX * NY * 2) + 1, -1., 1.)):
        with pytest.raises(E.EngineError):
            eng.render_field_cube(fields, widths, theta, phi, NX, NY, anchor,
                                  sides, nchan, lo, hi)
    assert np.array_equal(a, eng.render_field_cube(
        fields, widths, *args, extinction=k, velocity=vel))

    lex = lexington_engine(6)
    n = 216
    line_args = (0.7, 0.3, 9, 8, (-2.e17, -2.e17), (4.e17, 4.e17))
    with pytest.raises(E.EngineError, match="cell data"):
        lex.render_line_cube(["HAlpha"], *line_args, 4, -5.e4, 5.e4)
    density, temperature, x = random_state(6, 3)
    lex.upload_cells(density, temperature, x)
    rng = np.random.default_rng(61)
    v = rng.uniform(-2.e4, 2.e4, (3, n))
    at_rest = lex.render_line_cube(["HAlpha"], *line_args, 12, -5.e4, 5.e4)
    lex.set_cell_velocities(v)
    moving = lex.render_line_cube(["HAlpha"], *line_args, 12, -5.e4, 5.e4)
    assert moving["HAlpha"].any()
    assert not np.array_equal(moving["HAlpha"], at_rest["HAlpha"])
    for bad in (np.inf, -np.inf, np.nan):
        w = v.copy()
        w[1, 100] = bad
        with pytest.raises(E.EngineError, match="not finite"):
            lex.set_cell_velocities(w)
        # the previous state is kept
        again = lex.render_line_cube(["HAlpha"], *line_args, 12, -5.e4, 5.e4)
        assert np.array_equal(again["HAlpha"], moving["HAlpha"])
    for name in ("HII", "BALMER_JUMP_LOW", "avg_T", "Hrec_s", "WFC2_F555W"):
        with pytest.raises(E.EngineError, match="not the line of one ion"):
            lex.render_line_cube(["HAlpha", name], *line_args, 4, -5.e4,
                                 5.e4)
    for kwargs in (dict(sigma_turb=-1.), dict(sigma_turb=np.nan),
                   dict(sigma_turb=np.inf), dict(dust_cross_section=-1.e-30),
                   dict(supersample=0), dict(supersample=9)):
        with pytest.raises(E.EngineError):
            lex.render_line_cube(["HAlpha"], *line_args, 4, -5.e4, 5.e4,
                                 **kwargs)
    for nchan, lo, hi in ((0, -1., 1.), (4, 1., 1.), (4, 2., 1.),
                          (4, -np.inf, 1.), (4, 0., np.nan),
                          ((1 << 28) // 72 + 1, -1., 1.)):
        with pytest.raises(E.EngineError):
            lex.render_line_cube(["HAlpha"], *line_args, nchan, lo, hi)
    lex.set_cell_velocities(None)
    again = lex.render_line_cube(["HAlpha"], *line_args, 12, -5.e4, 5.e4)
    assert np.array_equal(again["HAlpha"], at_rest["HAlpha"])
    lex.set_cell_velocities(np.zeros((3, n)))
    again = lex.render_line_cube(["HAlpha"], *line_args, 12, -5.e4, 5.e4)
    assert np.array_equal(again["HAlpha"], at_rest["HAlpha"])
    # the engine still computes
    assert lex.compute_emissivities(["HAlpha"])["HAlpha"].max() > 0.
    lex.close()

    periodic = GpuEngine((4, 4, 4), (0., 0., 0.), (1., 1., 1.), (1, 0, 0),
                         device=0)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.render_field_cube(np.ones(64), np.ones(64), 0.3, 0.2, 4, 4,
                                   (-1., -1.), (2., 2.), 3, -1., 1.)
    periodic.close()
    block = GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                      device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    with pytest.raises(E.EngineError, match="decomposed"):
        block.render_field_cube(np.ones(64), np.ones(64), 0.3, 0.2, 4, 4,
                                (-1., -1.), (2., 2.), 3, -1., 1.)
    block.close()
