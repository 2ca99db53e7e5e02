"""Sky cubes on the device (cmi_gpu_render_field_sky_cube,
cmi_gpu_render_line_sky_cube, cmi_gpu_render_line_sky_map_cube; DESIGN.md
4.13) against the identities of the contract, against the CPU restatement
(tests/support/sky_cube_reference.c, checked on its own in
test_sky_cube_host.py), against the parallel camera's cubes and against
themselves."""
import numpy as np
import pytest

import sky_cube_lib as Q
import sky_image_lib as S
from test_gpu_emissivity import random_state
from test_gpu_line_cube import U_CPU, U_DEV
from test_gpu_line_image import lexington_box, plain_engine
from test_gpu_physics import lexington_engine
from test_gpu_sky_image import BOX, EXACT, probe_origins, sky_cases

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CB = Q.channel_block()
EINVAL = "error 1:"  # include/cmi_gpu.h, as GpuEngine._check words it
V0 = np.array([3., -5., 9.])


@pytest.fixture(scope="module")
def eng():
    engine = plain_engine(BOX)
    yield engine
    engine.close()


def random_cells(seed, nfields=2):
    """fields 10^U(-2, 1) with some dark cells, widths over a factor of 30
    with some cold cells (b == 0), |v| up to 32 b, extinction with optical
    depths per cell around 0.1 and some cells without dust (k == 0)"""
    rng = np.random.default_rng(seed)
    fields = 10. ** rng.uniform(-2., 1., (nfields, BOX.n))
    fields[rng.uniform(size=(nfields, BOX.n)) < 0.1] = 0.
    widths = 10. ** rng.uniform(0., np.log10(30.), (nfields, BOX.n))
    widths[rng.uniform(size=(nfields, BOX.n)) < 0.1] = 0.
    direction = rng.normal(size=(3, BOX.n))
    direction /= np.linalg.norm(direction, axis=0)
    speed = 32. * np.maximum(widths[0], 1.) * rng.uniform(0., 1., BOX.n)
    k = 10. ** rng.uniform(-1.5, 0.5, BOX.n)
    k[rng.uniform(size=BOX.n) < 0.1] = 0.
    return fields, widths, direction * speed, k


def steps_of(box, origin, d):
    return S.probe(box, origin, d, 0)[:, 2]


@pytest.mark.parametrize("nfields", [3, 8])
def test_identity_1_one_wide_channel_is_the_sky(eng, nfields):
    """Case 1: nchan = 1 over a range that covers u +- 6 b of every cell on
    every ray: f_0 = 0.5 * (1 - -1) = 1 and the cube is render_field_sky, bit
    for bit, from every origin and ray list, without and with dust; 8 fields
    are two batches of the cube's records (6 + 2) against two of the sky's (7
    + 1). The observer moves, so w is not v."""
    fields, widths, vel, k = random_cells(41, nfields)
    v_obs = np.array([12., -30., 7.])
    reach = (np.abs(vel).sum(axis=0).max() + np.abs(v_obs).sum() +
             6. * widths.max())
    rng = np.random.default_rng(2)
    for origin, d in sky_cases(BOX, rng):
        for ext in (None, k):
            sky = eng.render_field_sky(fields, origin, d, extinction=ext)
            cube = eng.render_field_sky_cube(
                fields, widths, origin, d, 1, -reach, reach, extinction=ext,
                velocity=vel, observer_velocity=v_obs)
            assert cube.shape == (nfields, 1, len(d))
            if len(d) > 1:
                assert (sky > 0.).sum() > 0.3 * sky.size
            assert np.array_equal(cube[:, 0], sky), (origin, len(d))
    # some rays miss: from outside
    origin, d = sky_cases(BOX, np.random.default_rng(2))[2]
    sky = eng.render_field_sky(fields, origin, d)
    assert (sky[0] == 0.).sum() > 400 and (sky[0] > 0.).sum() > 400


def test_more_rays_than_one_launch_takes(eng):
    """Case 1 across the chunks of rays: 2^22 + 1000 rays (CMI_SKY_LAUNCH_RAYS
    is 2^22) are two launches, and the planes of each come down one by one
    into their places among the call's rays. Two fields, nchan = 1 over a
    range that covers every cell: render_field_sky on the same rays, bit for
    bit, every ray in its place."""
    fields, widths, vel, _ = random_cells(53)
    reach = np.abs(vel).sum(axis=0).max() + 6. * widths.max()
    n = (1 << 22) + 1000
    origin = probe_origins(BOX)["inside"]
    d = S.random_directions(np.random.default_rng(7), n)
    sky = eng.render_field_sky(fields, origin, d)
    cube = eng.render_field_sky_cube(fields, widths, origin, d, 1, -reach,
                                     reach, velocity=vel)
    assert cube.shape == (2, 1, n) and sky.shape == (2, n)
    assert (sky[:, 1 << 22:] > 0.).any() and not np.array_equal(sky[0], sky[1])
    assert np.array_equal(cube[:, 0], sky)


@pytest.mark.parametrize("nchan", sorted({1, 5, CB, CB + 1, 2 * CB + 3}))
def test_parity_with_the_restatement(eng, nchan):
    """Case 2: per ray r of n_r steps and per channel c

      |gpu - cpu| <= eps (8 (n_r + 2) I_c + (U_dev + U_cpu + 4 slope) I_tot)

    First term, what is not f: a step adds T * ((s * emit) * f). On one side
    T is a product of n_r factors exp(-dtau), each within 2 ulp of the true
    value in either libm, and n_r roundings: 3 n_r eps; emit = -expm1 (2 ulp)
    times s, times f, times T: 5 eps more; the n_r additions of positive
    terms: n_r eps; 4 n_r + 5 per side, both sides: 8 n_r + 10 <= 8 (n_r +
    2), relative to the channel's value I_c. (dtau = k ds, ds and u are the
    same IEEE operations on the same bits on both sides - u = (w_x d_x + w_y
    d_y) + w_z d_z included - and add nothing.)
    Second term, f: E is wrong by at most U / 2 eps on either side (U ulps of
    a value below 1), f = 0.5 (E_hi - E_lo) by as much, together (U_dev +
    U_cpu) / 2 eps, taken twice as in the line cubes; the rounding of e - u
    and of the division by b shift z by 2 eps |z|, which erf's slope, at most
    2 / sqrt(pi), turns into less than 4 eps (|e| + |u|) / b, with |u| <=
    |w_x| + |w_y| + |w_z|. An error of f weighs T (s emit), whose sum over
    the ray is the integrated sky value I_tot.
    The range cuts through the emission on its lower side. No ray is left
    out."""
    fields, widths, vel, k = random_cells(43)
    v_obs = np.array([40., 0., -25.])
    vmin, vmax = -150., 1100.
    edges = Q.edges(nchan, vmin, vmax)
    w1 = np.abs(vel - v_obs[:, None]).sum(axis=0)
    warm = widths > 0.
    reach = np.broadcast_to(w1 + np.abs(edges).max(), widths.shape)
    slope = (reach[warm] / widths[warm]).max()
    worst = 0.
    rng = np.random.default_rng(4)
    for origin, d in sky_cases(BOX, rng):
        steps = steps_of(BOX, origin, d)
        for ext in (None, k):
            want = Q.render(BOX, fields, widths, origin, d, nchan, vmin, vmax,
                            extinction=ext, velocity=vel,
                            observer_velocity=v_obs)
            total = S.render(BOX, fields, origin, d, extinction=ext)
            got = eng.render_field_sky_cube(
                fields, widths, origin, d, nchan, vmin, vmax, extinction=ext,
                velocity=vel, observer_velocity=v_obs)
            assert got.shape == want.shape == (2, nchan, len(d))
            assert not np.isnan(got).any()
            if len(d) > 1:
                # the range cuts: part of the emission is outside it
                assert 0.2 * total.sum() < want.sum() < 0.98 * total.sum()
            bound = EPS * (8. * (steps + 2.) * want +
                           (U_DEV + U_CPU + 4. * slope) * total[:, None])
            diff = np.abs(got - want)
            dark = bound == 0.
            assert not got[dark].any() and not want[dark].any()
            ratio = (diff[~dark] / bound[~dark]).max()
            worst = max(worst, ratio)
            print("nchan", nchan, "rays", len(d), "dust", ext is not None,
                  "longest", int(steps.max()), "slope", slope,
                  "worst |gpu - cpu| / bound", ratio)
            assert (diff <= bound).all()
    print("nchan", nchan, "worst ratio of difference to bound", worst)


def dipole_setup():
    """a uniform velocity field with integer components, b == 0 everywhere;
    0 is an edge (2 CB channels of width 32 / (2 CB), a power of two)"""
    rng = np.random.default_rng(47)
    field = 10. ** rng.uniform(-2., 1., BOX.n)
    vel = np.repeat(V0[:, None], BOX.n, axis=1)
    origin = probe_origins(BOX)["inside"]
    d = np.concatenate([S.random_directions(rng, 2000),
                        S.special_directions()])
    return field, vel, origin, d, 2 * CB, -16., 16.


def test_the_sign_and_the_dipole(eng):
    """Case 3: ray r's whole sky value sits in the one channel that holds
    u_r = (v_0x d_x + v_0y d_y) + v_0z d_z, every other channel is exactly 0,
    and matter that recedes (v_0 . d > 0) lands at or above the edge 0, matter
    that approaches below it."""
    field, vel, origin, d, nchan, vmin, vmax = dipole_setup()
    sky = eng.render_field_sky(field, origin, d)[0]
    cube = eng.render_field_sky_cube(field, np.zeros(BOX.n), origin, d, nchan,
                                     vmin, vmax, velocity=vel)[0]
    assert (sky > 0.).all()
    u = Q.radial_velocity(V0, d)
    edges = Q.edges(nchan, vmin, vmax)
    channel = np.searchsorted(edges, u, side="right") - 1
    assert channel.min() >= 0 and channel.max() < nchan
    rays = np.arange(len(d))
    assert np.array_equal(cube[channel, rays], sky)
    rest = cube.copy()
    rest[channel, rays] = 0.
    assert not rest.any()
    zero = nchan // 2   # the channel whose lower edge is 0
    assert edges[zero] == 0.
    assert (channel[u > 0.] >= zero).all() and (channel[u < 0.] < zero).all()
    assert (u > 0.).sum() > 800 and (u < 0.).sum() > 800
    assert len(np.unique(channel)) > nchan // 2


def test_identity_2_and_the_observer(eng):
    """Case 4: integer velocities, so that every v - v_obs is exact: (v,
    v_obs), (v - v_obs, 0) and (v + a, v_obs + a) are the same call, bit for
    bit, and not the call without v_obs. An observer who moves with the
    uniform field of case 3 sees everything in the channel of 0."""
    fields, widths, _, k = random_cells(49)
    rng = np.random.default_rng(50)
    vel = rng.integers(-300, 301, (3, BOX.n)).astype(float)
    v_obs = np.array([17., -140., 60.])
    a = np.array([-4000., 250., 1.e5])
    origin = probe_origins(BOX)["inside"]
    d = np.concatenate([S.random_directions(rng, 1500),
                        S.special_directions()])
    args = (fields, widths, origin, d, 2 * CB + 3, -250., 400.)
    first = eng.render_field_sky_cube(*args, extinction=k, velocity=vel,
                                      observer_velocity=v_obs)
    assert (first > 0.).sum() > 0.3 * first.size
    assert np.array_equal(first, eng.render_field_sky_cube(
        *args, extinction=k, velocity=vel - v_obs[:, None]))
    assert np.array_equal(first, eng.render_field_sky_cube(
        *args, extinction=k, velocity=vel + a[:, None],
        observer_velocity=v_obs + a))
    assert not np.array_equal(first, eng.render_field_sky_cube(
        *args, extinction=k, velocity=vel))
    # velocity None is a field at rest
    assert np.array_equal(
        eng.render_field_sky_cube(*args, observer_velocity=v_obs),
        eng.render_field_sky_cube(*args, velocity=np.zeros((3, BOX.n)),
                                  observer_velocity=v_obs))

    field, vel, origin, d, nchan, vmin, vmax = dipole_setup()
    sky = eng.render_field_sky(field, origin, d)[0]
    cube = eng.render_field_sky_cube(field, np.zeros(BOX.n), origin, d, nchan,
                                     vmin, vmax, velocity=vel,
                                     observer_velocity=V0)[0]
    assert np.array_equal(cube[nchan // 2], sky)
    assert not np.delete(cube, nchan // 2, axis=0).any()


def test_identity_3_the_channels_sum_to_the_sky(eng):
    """Case 5: with a range that covers u +- 6 b of every cell the sum over
    channels is the sky value of the same ray within (nchan + 8 n_r) eps
    relative, the line cubes' bound: both sides are the device's own exp and
    expm1 on the same bits, so what differs is the nchan roundings of the
    fractions and of their sum and a few roundings per step. A narrower
    range gives less, and never more than that bound above the sky value."""
    fields, widths, vel, k = random_cells(53)
    v_obs = np.array([5., 9., -14.])
    reach = (np.abs(vel).sum(axis=0).max() + np.abs(v_obs).sum() +
             6. * widths.max())
    nchan = 2 * CB + 3
    rng = np.random.default_rng(6)
    for origin, d in sky_cases(BOX, rng):
        tol = (nchan + 8. * steps_of(BOX, origin, d)) * EPS
        for ext in (None, k):
            sky = eng.render_field_sky(fields, origin, d, extinction=ext)
            cube = eng.render_field_sky_cube(
                fields, widths, origin, d, nchan, -reach, reach,
                extinction=ext, velocity=vel, observer_velocity=v_obs)
            total = cube.sum(axis=1)
            lit = sky > 0.
            assert not total[~lit].any()
            err = np.abs(total - sky)
            print("rays", len(d), "dust", ext is not None, "worst / allowed",
                  (err[lit] / (tol * sky)[lit]).max())
            assert (err <= tol * sky).all()
            part = eng.render_field_sky_cube(
                fields, widths, origin, d, nchan, 0.02 * reach, 0.3 * reach,
                extinction=ext, velocity=vel,
                observer_velocity=v_obs).sum(axis=1)
            assert (part <= sky * (1. + tol)).all()
            if len(d) > 1:
                assert part.sum() < 0.75 * sky.sum()


def small_lexington(ncell, seed):
    density, temperature, x = random_state(ncell, seed)
    eng = lexington_engine(ncell)
    eng.upload_cells(density, temperature, x)
    return eng, density, temperature, x


def test_map_cube_is_the_ray_list_cube():
    """Case 6: the map call is the ray-list call on sky_map_directions' rays,
    bit for bit (24 x 12 pixels of a window in a turned frame, and the full
    sky at 13 x 9, no multiples of 8); cube_moments of it gives finite mean
    velocities wherever moment 0 is positive."""
    from cmacionize_amd import engine as E
    import oracle_lib as o
    ncell = 10
    eng, _, _, _ = small_lexington(ncell, 23)
    rng = np.random.default_rng(24)
    eng.set_cell_velocities(rng.uniform(-2.e4, 2.e4, (3, ncell ** 3)))
    lines = ["HAlpha", "OIII_5007"]
    origin = np.array([1., -0.5, 0.3]) * o.PC
    c, s = np.cos(0.4), np.sin(0.4)
    frame = np.array([[c, s, 0.], [0., 0., 1.], [s, -c, 0.]])
    nchan, vmin, vmax = CB + 3, -1.5e5, 1.4e5
    kw = dict(dust_cross_section=2.e-27, sigma_turb=3.e3,
              observer_velocity=(4.e3, -1.e3, 8.e3))
    for nlon, nlat, window in (
            (24, 12, dict(lon_range=(0.2, 1.7), lat_range=(-0.3, 0.9),
                          frame=frame)), (13, 9, {})):
        d, _ = E.sky_map_directions(nlon, nlat, **window)
        rays = eng.render_line_sky_cube(lines, origin, d, nchan, vmin, vmax,
                                        **kw)
        maps = eng.render_line_sky_map_cube(lines, origin, nlon, nlat, nchan,
                                            vmin, vmax, **window, **kw)
        assert list(maps) == lines
        centres = E.cube_channel_centres(nchan, vmin, vmax)
        for name in lines:
            assert maps[name].shape == (nchan, nlon, nlat)
            assert rays[name].shape == (nchan, nlon * nlat)
            assert np.array_equal(maps[name].reshape(nchan, -1), rays[name])
            m0, mean, disp = E.cube_moments(maps[name], centres)
            assert (m0 > 0.).mean() > 0.9
            assert np.isfinite(mean[m0 > 0.]).all()
            assert (np.abs(mean[m0 > 0.]) < 1.5e5).all()
        # the range covers everything: the integrated map
        sky = eng.render_line_sky_map(lines, origin, nlon, nlat,
                                      dust_cross_section=2.e-27, **window)
        assert np.allclose(maps["HAlpha"].sum(axis=0), sky["HAlpha"],
                           rtol=1e-9)
    eng.close()


def test_sky_cube_end_to_end(oracle):
    """Case 7: the random lexington state of the line-cube test with a radial
    expansion about the observer, who sits inside the box and moves: H alpha
    and [O III] 5007 in one call against the restatement fed with the
    oracle's emissivities and with widths from the table of atomic weights
    in numpy, within that test's 2e-10 of the ray's integrated brightness
    (what an emissivity's own difference scales with). With sigma_turb = 0
    and one temperature the [O III] line is narrower than H alpha by
    sqrt(15.9994 / 1.00794)."""
    import oracle_lib as o
    from cmacionize_amd import engine as E
    ncell = 12
    sim = oracle.lexington_simulation(ncell)
    eng, density, temperature, x = small_lexington(ncell, 7)
    box = lexington_box(ncell)
    n = ncell ** 3
    names = ["HAlpha", "OIII_5007"]
    ref = np.array([oracle.emissivities(sim.model, density[c], temperature[c],
                                        x[:, c]) for c in range(n)]).T
    ref = ref[[E.EMISSION_LINES.index(name) for name in names]]
    origin = np.array([1., -0.5, 0.3]) * o.PC
    idx = np.stack(np.meshgrid(*[np.arange(ncell)] * 3, indexing="ij"))
    r = (box.anchor[:, None] + (idx.reshape(3, n) + 0.5) *
         box.cellside[:, None])
    vel = 15.e3 * (r - origin[:, None]) / (5. * o.PC)
    eng.set_cell_velocities(vel)
    v_obs = np.array([2.e3, -3.e3, 1.e3])
    k_B, m_u = 1.38064852e-23, 1.660539040e-27
    rng = np.random.default_rng(12)
    d = S.random_directions(rng, 700)
    nchan, vmin, vmax = 96, -48.e3, 48.e3
    for turb in (0., 4.e3):
        widths = np.array([np.sqrt(2. * (k_B * temperature /
                                         (E.LINE_ATOMIC_WEIGHTS[name] * m_u) +
                                         turb * turb)) for name in names])
        for sigma in (0., 2.e-27):
            ext = density * sigma if sigma else None
            got = eng.render_line_sky_cube(names, origin, d, nchan, vmin,
                                           vmax, sigma, turb, v_obs)
            assert list(got) == names
            want = Q.render(box, ref, widths, origin, d, nchan, vmin, vmax,
                            extinction=ext, velocity=vel,
                            observer_velocity=v_obs)
            total = S.render(box, ref, origin, d, extinction=ext)
            for l, name in enumerate(names):
                assert got[name].shape == (nchan, len(d))
                assert (total[l] > 0.).all()
                err = (np.abs(got[name] - want[l]) / total[l]).max()
                print(name, "dust", sigma, "turb", turb, "worst / I_tot", err)
                assert err < 2.e-10, (name, sigma, err)
            # the expansion is about the observer: everything recedes
            # (but for the observer's own 3.7 km/s), the mean is positive
            centres = E.cube_channel_centres(nchan, vmin, vmax)
            _, mean, _ = E.cube_moments(got["HAlpha"][:, :, None], centres)
            assert (mean > 0.).mean() > 0.9
    eng.upload_cells(density, np.full(n, 8000.), x)
    eng.set_cell_velocities(None)
    still = eng.render_line_sky_cube(names, origin, d[:50], 480, vmin, vmax)
    centres = E.cube_channel_centres(480, vmin, vmax)
    m0_h, _, disp_h = E.cube_moments(still["HAlpha"][:, :, None], centres)
    m0_o, _, disp_o = E.cube_moments(still["OIII_5007"][:, :, None], centres)
    ray = np.unravel_index(np.argmax(m0_o), m0_o.shape)
    assert m0_h[ray] > 0. and m0_o[ray] > 0.
    ratio = disp_h[ray] / disp_o[ray]
    expect = np.sqrt(15.9994 / 1.00794)
    print("dispersions", disp_h[ray], disp_o[ray], "ratio", ratio,
          "expected about", expect)
    assert abs(ratio / expect - 1.) < 0.05
    eng.close()


def test_against_the_parallel_camera():
    """Case 8: one ray from far outside along -z through a column of EXACT
    (walls, origin and entry point are exact doubles, every ds is 0.5) and
    the parallel cube at theta = 0 of the one pixel whose sample ray is that
    column, without dust: n = (0, 0, 1) there and d = (0, 0, -1) here, so u =
    -v_z in both contracts, and a channel holds the same addends (s ds) f_c
    in the opposite order: within (steps + 2) eps of the channel's value."""
    eng = plain_engine(EXACT)
    fields, widths, vel, _ = random_cells(61)
    wx, wy, h = 0.375, 1.0625, 0.03125   # the column (5, 4, .)'s middle
    top = EXACT.anchor[2] + EXACT.sides[2]
    origin = np.array([wx, wy, top + 64.])
    d = np.array([[0., 0., -1.]])
    nchan, vmin, vmax = 2 * CB + 3, -700., 500.
    sky = eng.render_field_sky_cube(fields, widths, origin, d, nchan, vmin,
                                    vmax, velocity=vel)[:, :, 0]
    # theta = phi = 0: image x is the world's y, image y the world's -x
    par = eng.render_field_cube(fields, widths, 0., 0., 1, 1,
                                (wy - h, -wx - h), (2. * h, 2. * h), nchan,
                                vmin, vmax, velocity=vel)[:, :, 0, 0]
    steps = int(S.probe(EXACT, origin, d, 0)[0, 2])
    assert steps == EXACT.ncell[2]
    # the column is the one meant: cells (5, 4, 13 .. 0)
    rows = S.probe(EXACT, origin, d, steps)[0]
    cells = (5 * EXACT.ncell[1] + 4) * EXACT.ncell[2] + np.arange(13, -1, -1)
    assert np.array_equal(rows[3:3 + steps], cells)
    assert (rows[3 + steps:] == 0.5).all()
    assert (sky > 0.).sum() > 6 and (sky == 0.).any()
    tol = (steps + 2) * EPS * np.maximum(sky, par)
    print("worst / allowed", (np.abs(sky - par)[tol > 0.] / tol[tol > 0.]).max())
    assert (np.abs(sky - par) <= tol).all()
    # and it is a sign that is tested: the mirrored velocities differ
    flipped = eng.render_field_sky_cube(fields, widths, origin, d, nchan, vmin,
                                        vmax, velocity=-vel)[:, :, 0]
    assert (np.abs(flipped - par) > 1e3 * tol).any()
    eng.close()


def test_repeats_and_refusals(eng):
    """Case 9: the same call twice gives the same bits; every refusal is
    EINVAL, and after each the good call gives the bits it gave before."""
    from cmacionize_amd import GpuEngine
    from cmacionize_amd import engine as E
    fields, widths, vel, k = random_cells(59)
    origin = probe_origins(BOX)["inside"]
    rng = np.random.default_rng(60)
    d = S.random_directions(rng, 1000)
    v_obs = (1., 2., 3.)
    nchan, lo, hi = CB + 3, -300., 700.

    def call(f=fields, w=widths, o=origin, dirs=d, n=nchan, a=lo, b=hi, **kw):
        kw.setdefault("extinction", k)
        kw.setdefault("velocity", vel)
        kw.setdefault("observer_velocity", v_obs)
        return eng.render_field_sky_cube(f, w, o, dirs, n, a, b, **kw)

    good = call()
    assert good.any() and np.array_equal(good, call())
    nan, inf = float("nan"), float("inf")
    bad_d = d.copy()
    bad_d[17] *= 1.001
    bad_w = widths.copy()
    bad_w[1, 17] = -1.
    bad_v = vel.copy()
    bad_v[2, 5] = inf
    refused = [dict(n=0), dict(n=-2), dict(a=1., b=1.), dict(a=2., b=1.),
               dict(a=nan), dict(b=nan), dict(a=-inf), dict(a=-1.e308,
                                                            b=1.e308),
               dict(observer_velocity=(0., nan, 0.)),
               dict(observer_velocity=(inf, 0., 0.)), dict(dirs=bad_d),
               dict(w=bad_w), dict(velocity=bad_v),
               dict(o=(0., nan, 0.)),
               dict(n=(1 << 28) // (2 * len(d)) + 1)]
    for kw in refused:
        with pytest.raises(E.EngineError, match=EINVAL):
            call(**kw)
        assert np.array_equal(good, call()), kw
    with pytest.raises(E.EngineError, match="2\\^28"):
        call(n=(1 << 28) // (2 * len(d)) + 1)

    lex, _, _, _ = small_lexington(6, 3)
    n = 216
    v = rng.uniform(-2.e4, 2.e4, (3, n))
    lex.set_cell_velocities(v)
    o6 = (1.e16, -2.e16, 3.e16)
    line_args = (o6, d[:100], 12, -5.e4, 5.e4)
    moving = lex.render_line_sky_cube(["HAlpha"], *line_args)["HAlpha"]
    assert moving.any()
    for name in ("HII", "BALMER_JUMP_LOW", "avg_T", "Hrec_s", "WFC2_F555W"):
        with pytest.raises(E.EngineError, match="not the line of one ion"):
            lex.render_line_sky_cube(["HAlpha", name], *line_args)
    for kw in (dict(sigma_turb=-1.), dict(sigma_turb=nan),
               dict(dust_cross_section=-1.e-30),
               dict(observer_velocity=(nan, 0., 0.))):
        with pytest.raises(E.EngineError, match=EINVAL):
            lex.render_line_sky_cube(["HAlpha"], *line_args, **kw)
    with pytest.raises(E.EngineError, match=EINVAL):
        lex.render_line_sky_cube(["HAlpha"], o6, d[:100],
                                 (1 << 28) // 100 + 1, -5.e4, 5.e4)
    for kw in (dict(nlon=0), dict(lat_range=(-2., 1.)),
               dict(nchan=0), dict(observer_velocity=(0., 0., nan))):
        args = dict(nlon=8, nlat=4, nchan=3, vmin=-5.e4, vmax=5.e4)
        args.update(kw)
        with pytest.raises(E.EngineError, match=EINVAL):
            lex.render_line_sky_map_cube(["HAlpha"], o6, **args)
    # a failed call leaves the velocities as they were
    again = lex.render_line_sky_cube(["HAlpha"], *line_args)["HAlpha"]
    assert np.array_equal(again, moving)
    lex.set_cell_velocities(None)
    rest = lex.render_line_sky_cube(["HAlpha"], *line_args)["HAlpha"]
    assert rest.any() and not np.array_equal(rest, moving)
    fresh = lexington_engine(6)
    with pytest.raises(E.EngineError, match="cell data"):
        fresh.render_line_sky_cube(["HAlpha"], *line_args)
    fresh.close()
    lex.close()

    periodic = GpuEngine((4, 4, 4), (0., 0., 0.), (1., 1., 1.), (1, 0, 0),
                         device=0)
    with pytest.raises(E.EngineError, match=EINVAL + ".*periodic"):
        periodic.render_field_sky_cube(np.ones(64), np.ones(64),
                                       (0.5, 0.5, 0.5), (0., 0.6, 0.8), 3,
                                       -1., 1.)
    periodic.close()
    block = GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                      device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    with pytest.raises(E.EngineError, match="decomposed"):
        block.render_field_sky_cube(np.ones(64), np.ones(64), (0.5, 0.5, 0.5),
                                    (0., 0.6, 0.8), 3, -1., 1.)
    block.close()
