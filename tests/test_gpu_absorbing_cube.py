"""Absorbing line cubes on the device (include/cmi_gpu.h, "absorbing line
cubes") through the C ABI: the contract's exact identities,
the independence of a channel from its block, its chunk and the shortcut for
dark cells, velocity-shift invariance, parity with the CPU restatement
(tests/support/absorbing_cube_reference.c, checked on its own in
test_absorbing_cube_host.py) within a derived bound, the probe, the 21-cm
coefficients against their numpy form, and the refusals."""
import numpy as np
import pytest

import absorbing_cube_lib as A
import continuum_lib as K
import line_image_lib as L

pytestmark = pytest.mark.gpu

EPS = A.EPS
BOX, NX, NY, VIEWS = A.BOX, A.NX, A.NY, A.VIEWS
SUPERSAMPLE = (1, 2, 1, 2, 1, 2)   # per view
CB = A.channel_block()
EINVAL, ESTATE = 1, 3  # include/cmi_gpu.h
DV = 2.


def axis_of(nchan):
    """nchan channels of width DV with an edge at exactly 0"""
    vmin = -DV * (nchan // 2)
    return nchan, vmin, vmin + DV * nchan


@pytest.fixture(scope="module")
def eng():
    from cmacionize_amd import GpuEngine
    engine = GpuEngine(tuple(int(n) for n in BOX.ncell), tuple(BOX.anchor),
                       tuple(BOX.sides), (0, 0, 0), device=0)
    yield engine
    engine.close()


@pytest.fixture(scope="module")
def cells():
    """random cells, shared and left unchanged: {a, sl, b, velocity, kc, sc}
    and a background"""
    a, sl, b, vel, kc, sc = A.random_cells(BOX, 101, DV)
    bg = np.array(0.8 * sl.mean())
    for x in (a, sl, b, vel, kc, sc, bg):
        x.setflags(write=False)
    return dict(a=a, sl=sl, b=b, velocity=vel, kc=kc, sc=sc, background=bg)


def rectangle(view):
    return A.image_rectangle(BOX, *VIEWS[view])


def gpu_cube(eng, q, view, nchan, vmin, vmax, s=1, **more):
    theta, phi = VIEWS[view]
    anchor, sides = rectangle(view)
    f = dict(q, **more)
    return eng.render_field_absorbing_cube(
        f["a"], f["sl"], f["b"], theta, phi, NX, NY, anchor, sides, nchan,
        vmin, vmax, s, velocity=f["velocity"], kc=f["kc"], sc=f["sc"],
        background=f["background"])


def gpu_sky(eng, q, origin, d, nchan, vmin, vmax, **more):
    f = dict(q, **more)
    return eng.render_field_absorbing_sky_cube(
        f["a"], f["sl"], f["b"], origin, d, nchan, vmin, vmax,
        velocity=f["velocity"], kc=f["kc"], sc=f["sc"],
        background=f["background"],
        observer_velocity=f.get("observer_velocity"))


# ------------------------------------------------------------ 1 identities --

def test_exact_identities(eng, cells):
    """a == 0: every channel is the continuum call of {kc, sc} with nf = 1,
    bit for bit, for both cameras at supersampling 1 and 2; sl == sc == bg
    stays bg (parallel camera); a second call gives the bits of the first; a
    channel does not depend on how many channels the cube has"""
    nchan, vmin, vmax = axis_of(5)
    bg = cells["background"]
    zero = np.zeros(BOX.n)
    flat = np.full(BOX.n, float(bg))
    for view, (theta, phi) in enumerate(VIEWS):
        anchor, sides = rectangle(view)
        for s in (1, 2):
            want = eng.render_field_continuum_images(
                cells["kc"], cells["sc"], theta, phi, NX, NY, anchor, sides,
                s, background=bg)
            got = gpu_cube(eng, cells, view, nchan, vmin, vmax, s, a=zero)
            assert got.shape == (nchan, NX, NY)
            for c in range(nchan):
                assert np.array_equal(got[c], want[0]), (theta, phi, s, c)
            one = gpu_cube(eng, cells, view, nchan, vmin, vmax, s)
            two = gpu_cube(eng, cells, view, nchan, vmin, vmax, s)
            assert np.array_equal(one, two) and not np.isnan(one).any()
            assert len(np.unique(one)) > 100
            assert np.abs(one[2] - one[0]).max() > 0.
        got = gpu_cube(eng, cells, view, nchan, vmin, vmax, 1, sl=flat,
                       sc=flat)
        assert np.array_equal(got, np.full(got.shape, float(bg)))
        short = gpu_cube(eng, cells, view, CB + 1, vmin, vmin + (CB + 1) * DV)
        long = gpu_cube(eng, cells, view, 2 * CB + 3, vmin,
                        vmin + (2 * CB + 3) * DV)
        assert np.array_equal(short, long[:CB + 1])
    d = A.sky_directions()
    vo = (1., -2., 0.5)
    for origin in A.sky_origins(BOX):
        want = eng.render_field_continuum_sky(cells["kc"], cells["sc"],
                                              origin, d, background=bg)
        got = gpu_sky(eng, cells, origin, d, nchan, vmin, vmax, a=zero,
                      observer_velocity=vo)
        for c in range(nchan):
            assert np.array_equal(got[c], want[0]), (origin, c)
        one = gpu_sky(eng, cells, origin, d, nchan, vmin, vmax,
                      observer_velocity=vo)
        two = gpu_sky(eng, cells, origin, d, nchan, vmin, vmax,
                      observer_velocity=vo)
        assert np.array_equal(one, two) and not np.isnan(one).any()
        short = gpu_sky(eng, cells, origin, d, CB + 1, vmin,
                        vmin + (CB + 1) * DV)
        long = gpu_sky(eng, cells, origin, d, 2 * CB + 3, vmin,
                       vmin + (2 * CB + 3) * DV)
        assert np.array_equal(short, long[:CB + 1])
    # without a background and without a continuum: a ray that misses is 0
    got = gpu_cube(eng, cells, 3, nchan, vmin, vmax, background=None,
                   kc=None, sc=None)
    assert (got == 0.).sum() > 20 * nchan and (got > 0.).any()


# ------------------------------------------------- 2 block independence --

def test_block_chunk_and_window_independence(eng, cells):
    """the same bits for both block widths, with expm1 inlined and called,
    with and without the shortcut for dark cells, and across the chunk
    boundary of the sample rows and rays. The band starts above most line
    centres, so that its later blocks are dark for many cells."""
    nchan, vmin, vmax = 2 * CB + 3, 3. * DV, 3. * DV + (2 * CB + 3) * DV
    origin = A.sky_origins(BOX)[0]
    d = A.sky_directions()

    def both(s=2):
        return (gpu_cube(eng, cells, 3, nchan, vmin, vmax, s),
                gpu_sky(eng, cells, origin, d, nchan, vmin, vmax,
                        observer_velocity=(0.5, 0., -1.)))

    full_img, full_sky = both()
    # (cells that are dark for the whole band whatever the direction, and
    # cells that are dark for the band's last block of four channels)
    u = np.abs(cells["velocity"]).sum(axis=0)
    assert (u + 6. * cells["b"] < vmin).mean() > 0.03
    assert (u + 6. * cells["b"] < vmax - 4. * DV).mean() > 0.3
    try:
        for width in (4, 8):
            for call in (0, 1):
                for skip in (0, 1):
                    eng.set_tuning(absorbing_cube_channel_block=width,
                                   absorbing_cube_expm1_call=call,
                                   absorbing_cube_window_skip=skip)
                    img, sk = both()
                    assert np.array_equal(img, full_img), (width, call, skip)
                    assert np.array_equal(sk, full_sky), (width, call, skip)
        eng.set_tuning(absorbing_cube_channel_block=CB,
                       absorbing_cube_expm1_call=1,
                       absorbing_cube_window_skip=1)
        # 2 * NY * 2 = 68 sample rays per pixel row: chunks of 2 rows of
        # pixels (23 rows: a last chunk of one), and of 1; 100 rays per
        # launch (500 rays: full chunks), and 64 and 333 (a partial last)
        for launch in (2 * 68, 1, 100, 64, 333):
            eng.set_tuning(absorbing_cube_launch_rays=launch)
            img, sk = both()
            assert np.array_equal(img, full_img), launch
            assert np.array_equal(sk, full_sky), launch
    finally:
        eng.set_tuning(absorbing_cube_channel_block=CB,
                       absorbing_cube_expm1_call=1,
                       absorbing_cube_window_skip=1,
                       absorbing_cube_launch_rays=0)
    with pytest.raises(Exception, match="4 or 8"):
        eng.set_tuning(absorbing_cube_channel_block=16)


# ------------------------------------------------------ 3 velocity shift --

def test_velocity_shift_invariance(eng, cells):
    """theta = 0 (n = (0, 0, 1) exactly), velocities along z and edges in
    multiples of 2^-3: D = 40 added to every u and to the range leaves every
    e - u, hence the cube, as it is; the same for a ray along +z from a point,
    through the observer's velocity"""
    rng = np.random.default_rng(47)
    vz = np.round(rng.uniform(-12., 12., BOX.n) * 8.) / 8.
    vel = np.zeros((3, BOX.n))
    vel[2] = vz
    D = 40.
    shifted = vel.copy()
    shifted[2] -= D       # u = -v_z
    nchan, vmin, vmax = 9, -9., 9.
    one = gpu_cube(eng, cells, 0, nchan, vmin, vmax, 2, velocity=vel)
    two = gpu_cube(eng, cells, 0, nchan, vmin + D, vmax + D, 2,
                   velocity=shifted)
    assert np.array_equal(one, two)
    assert np.abs(one[4] - one[0]).max() > 0.
    origin = BOX.anchor + BOX.sides * np.array([0.37, 0.52, 0.11])
    up = np.array([[0., 0., 1.]])
    one = gpu_sky(eng, cells, origin, up, nchan, vmin, vmax, velocity=vel)
    two = gpu_sky(eng, cells, origin, up, nchan, vmin + D, vmax + D,
                  velocity=vel, observer_velocity=(0., 0., -D))
    assert np.array_equal(one, two) and (one > 0.).all()


# --------------------------------------------------------------- 4 parity --

@pytest.mark.parametrize("nchan", [1, 5, 8, 9, 19])
def test_parity_with_the_restatement(eng, cells, nchan):
    """|gpu - cpu| <= march_bound (absorbing_cube_lib has the derivation: the
    roundings of the contract's operations, the 2 ulps between the two expm1
    and the 5 ulps between the two erf carried through kappa and w, per
    crossing), in all six views at supersampling 1 and 2 and for rays from
    three origins; a ds / dv and kc ds per cell span 1e-12 to 50 with a tenth
    of the cells at exactly 0 each, b from 0 (delta lines, on channel edges
    and off them) to four channels"""
    nchan, vmin, vmax = axis_of(nchan)
    ds = BOX.cellside.mean()
    tau = cells["a"] / DV * ds
    assert (tau == 0.).mean() > 0.05 and tau.max() > 40.
    assert tau[tau > 0.].min() < 1e-11
    cold = cells["b"] == 0.
    on_edge = cold & ~cells["velocity"].any(axis=0)
    assert on_edge.sum() > 20 and (cold & ~on_edge).sum() > 20
    depth = A.line_depth(BOX, cells["a"], DV)
    bg = cells["background"]
    worst = 0.
    for view, ((theta, phi), s) in enumerate(zip(VIEWS, SUPERSAMPLE)):
        anchor, sides = rectangle(view)
        want = A.cube(BOX, cells["a"], cells["sl"], cells["b"], theta, phi,
                      NX, NY, anchor, sides, nchan, vmin, vmax, s,
                      velocity=cells["velocity"], kc=cells["kc"],
                      sc=cells["sc"], background=bg)
        steps = A.longest_ray
        got = gpu_cube(eng, cells, view, nchan, vmin, vmax, s)
        assert got.shape == want.shape and not np.isnan(got).any()
        bound = A.march_bound(steps, depth, cells["sl"], cells["sc"], bg,
                              supersample=s)
        ratio = np.abs(got - want).max() / bound
        print("nchan", nchan, "view", theta, phi, "s", s, "steps", steps,
              "|gpu - cpu| / bound", ratio)
        worst = max(worst, ratio)
        assert ratio <= 1., (theta, phi, s, ratio)
    print("parallel, nchan %d: largest |gpu - cpu| / bound %.3g" %
          (nchan, worst))
    worst = 0.
    vo = (1.5, -0.5, 2.)
    for origin in A.sky_origins(BOX):
        d = A.sky_directions(box=BOX, origin=origin)
        want = A.sky_cube(BOX, cells["a"], cells["sl"], cells["b"], origin, d,
                          nchan, vmin, vmax, velocity=cells["velocity"],
                          kc=cells["kc"], sc=cells["sc"], background=bg,
                          observer_velocity=vo)
        steps = A.longest_ray
        got = gpu_sky(eng, cells, origin, d, nchan, vmin, vmax,
                      observer_velocity=vo)
        assert got.shape == want.shape and not np.isnan(got).any()
        assert (want != bg).mean() > 0.4
        bound = A.march_bound(steps, depth, cells["sl"], cells["sc"], bg,
                              point=True)
        ratio = np.abs(got - want).max() / bound
        worst = max(worst, ratio)
        assert ratio <= 1., (origin, ratio)
    print("point, nchan %d: largest |gpu - cpu| / bound %.3g" % (nchan, worst))


# ---------------------------------------------------------------- 5 probe --

def test_probe_traces(eng, cells):
    """the (cell, ds) lists equal the restatement's exactly, the running I_c
    agrees within the bound of its step count, I_end is the render call's
    (the probe has no shortcut for dark cells, the render call has)"""
    m, (nchan, vmin, vmax) = 40, axis_of(5)
    theta, phi = VIEWS[4]
    anchor, sides = rectangle(4)
    xy = L.sample_coordinates(NX, NY, anchor, sides).reshape(-1, 2)
    vo = (1.5, -0.5, 2.)
    cases = [(dict(theta=theta, phi=phi), xy, False)]
    for origin in A.sky_origins(BOX):
        cases.append((dict(origin=origin, observer_velocity=vo),
                      A.sky_directions(box=BOX, origin=origin), True))
    depth = A.line_depth(BOX, cells["a"], DV)
    f = {k: cells[k] for k in ("velocity", "kc", "sc", "background")}
    for where, rays, point in cases:
        got = eng.absorbing_cube_probe(cells["a"], cells["sl"], cells["b"],
                                       rays, m, nchan, vmin, vmax, **where,
                                       **f)
        want = A.probe(BOX, cells["a"], cells["sl"], cells["b"], rays, m,
                       nchan, vmin, vmax, **where, **f)
        gt, gsteps, gcells, gds, gI, gend = A.split_probe(got, nchan, m)
        wt, wsteps, wcells, wds, wI, wend = A.split_probe(want, nchan, m)
        assert np.array_equal(gt, wt, equal_nan=True)
        assert np.array_equal(gsteps, wsteps) and gsteps.max() <= m
        assert (gsteps > 10).any()
        if not point:
            assert (gsteps == 0).any()      # the margin: rays that miss
        assert np.array_equal(gcells, wcells) and np.array_equal(gds, wds)
        step = np.arange(1, m + 1)
        per = np.array([A.march_bound(k, depth, cells["sl"], cells["sc"],
                                      cells["background"], point=point)
                        for k in step])
        assert (np.abs(gI - wI) <= per[None, None, :]).all()
        assert (np.abs(gend - wend) <=
                per[np.maximum(gsteps, 1) - 1][:, None]).all()
        if point:
            render = gpu_sky(eng, cells, where["origin"], rays, nchan, vmin,
                             vmax, observer_velocity=vo)
        else:
            render = gpu_cube(eng, cells, 4, nchan, vmin,
                              vmax).reshape(nchan, -1)
        assert np.array_equal(gend.T, render)


# --------------------------------------------------------- 6 coefficients --

def lattice():
    """cells: vacuum, fully ionized, T = 0, and T from 50 to 3e4 K at three
    densities and three ionization states; padded to the box with vacuum"""
    rows = [(0., 1e4, 1., 1.), (1e8, 1e4, 0., 0.), (1e8, 0., 1., 1.)]
    for T in (50., 100., 1e3, 7.5e3, 1e4, 3e4):
        for n in (1e6, 1e8, 3.3e10):
            for xH, xHe in ((1., 1.), (1e-3, 0.4), (0.5, 1.)):
                rows.append((n, T, xH, xHe))
    rows = np.array(rows).T
    cells = np.zeros((4, BOX.n))
    cells[1] = 1e4
    cells[:, :rows.shape[1]] = rows
    return cells, rows.shape[1]


def test_hi_coefficients_and_calls(eng):
    """hi_coefficients against the numpy form: a is the same IEEE operations
    (0 ulps); b has the device's sqrt, within 1 ulp (2 EPS); sl = A / expm1(x)
    has the two expm1 (4 EPS between them) and the division's rounding on
    either side, 6 EPS; {kc, sc} are the bits of free_free_coefficients at
    nu_10 (the same device function). The special cells give a == 0 exactly.
    The H I calls are the general calls of these coefficients, bit for bit."""
    from cmacionize_amd import engine as E
    state, used = lattice()
    n, T, xH, xHe = state
    x = np.zeros((E.NION, BOX.n))
    x[0], x[1] = xH, xHe
    helium = 0.1
    eng.set_abundances([helium, 0., 0., 0., 0., 0.])
    eng.upload_cells(n, T, x)
    rng = np.random.default_rng(5)
    per_cell = rng.uniform(20., 200., BOX.n)
    per_cell[5] = 0.
    per_cell[6] = -3.
    kappa, source = eng.free_free_coefficients([E.HI_FREQUENCY])
    for spin in (None, 120., per_cell):
        got = eng.hi_coefficients(sigma_turb=300., spin_temperature=spin)
        want = A.hi_coefficients(n, T, xH, xHe, helium, 300., spin)
        assert np.array_equal(got["a"], want["a"])
        assert (got["a"][:3] == 0.).all() and (got["a"][used:] == 0.).all()
        assert (got["a"][3:used] > 0.).sum() >= used - 5
        assert (np.abs(got["b"] - want["b"]) <= 2. * EPS * want["b"]).all()
        assert (np.abs(got["sl"] - want["sl"]) <= 6. * EPS * want["sl"]).all()
        assert np.array_equal(got["kc"], kappa[0])
        assert np.array_equal(got["sc"], source[0])
        assert all(np.isfinite(v).all() for v in got.values())
        print("spin", type(spin).__name__, "b within %.2f ulp, sl within "
              "%.2f ulp" % (
                  (np.abs(got["b"] / want["b"] - 1.)).max() / (2 * EPS),
                  np.nanmax(np.abs(got["sl"][want["sl"] > 0.] /
                                   want["sl"][want["sl"] > 0.] - 1.)) /
                  (2 * EPS)))
    if spin is per_cell:
        assert got["a"][5] == 0. and got["a"][6] == 0. and got["sl"][5] == 0.
    off = eng.hi_coefficients(free_free=False)
    assert not off["kc"].any() and not off["sc"].any()
    # the calls: velocities, a spin temperature, a background
    vel = rng.normal(size=(3, BOX.n)) * 2e3
    eng.set_cell_velocities(vel)
    q = eng.hi_coefficients(sigma_turb=300., spin_temperature=120.)
    bg = A.host_planck(2.725)
    nchan, vmin, vmax = 11, -8e3, 9e3
    theta, phi = VIEWS[3]
    anchor, sides = rectangle(3)
    want = eng.render_field_absorbing_cube(
        q["a"], q["sl"], q["b"], theta, phi, NX, NY, anchor, sides, nchan,
        vmin, vmax, 2, velocity=vel, kc=q["kc"], sc=q["sc"], background=bg)
    got = eng.render_hi_cube(theta, phi, NX, NY, anchor, sides, nchan, vmin,
                             vmax, 2, sigma_turb=300., spin_temperature=120.,
                             background_temperature=2.725)
    assert np.array_equal(got, want) and len(np.unique(got)) > 100
    origin = A.sky_origins(BOX)[0]
    vo = (500., -200., 100.)
    d, _ = E.sky_map_directions(16, 9)
    want = eng.render_field_absorbing_sky_cube(
        q["a"], q["sl"], q["b"], origin, d.reshape(-1, 3), nchan, vmin, vmax,
        velocity=vel, kc=q["kc"], sc=q["sc"], background=bg,
        observer_velocity=vo)
    got = eng.render_hi_sky_cube(origin, d.reshape(-1, 3), nchan, vmin, vmax,
                                 sigma_turb=300., spin_temperature=120.,
                                 background_temperature=2.725,
                                 observer_velocity=vo)
    maps = eng.render_hi_sky_map_cube(origin, 16, 9, nchan, vmin, vmax,
                                      sigma_turb=300., spin_temperature=120.,
                                      background_temperature=2.725,
                                      observer_velocity=vo)
    assert np.array_equal(got, want)
    assert np.array_equal(maps.reshape(nchan, -1), got)
    eng.set_cell_velocities(None)


# ------------------------------------------------------------ 7 refusals --

def test_refusals(eng, cells):
    from cmacionize_amd import engine as E
    theta, phi = VIEWS[3]
    anchor, sides = rectangle(3)
    d = A.sky_directions()[:10]
    origin = A.sky_origins(BOX)[0]
    lib, h = eng._lib, eng._h
    p = A._p
    # (the H I calls' own refusals come after the one for missing cells)
    eng.upload_cells(np.full(BOX.n, 1e8), np.full(BOX.n, 100.),
                     np.ones((E.NION, BOX.n)))
    base = {k: A._f64(cells[k]).copy() for k in
            ("a", "sl", "b", "velocity", "kc", "sc")}
    base["background"] = np.full(3, float(cells["background"]))

    def pointers(f):
        return [None if f[k] is None else p(f[k]) for k in
                ("a", "sl", "b", "velocity", "kc", "sc", "background")]

    def cube_call(nchan=3, vmin=-3., vmax=3., nx=NX, theta=theta, s=1, **f):
        f = dict(base, **f)
        out = np.full((3, NX, NY), -7.)
        rc = lib.cmi_gpu_render_field_absorbing_cube(
            h, *pointers(f), theta, phi, nx, NY, p(A._f64(anchor)),
            p(A._f64(sides)), s, nchan, vmin, vmax, p(out))
        return rc, lib.cmi_gpu_last_error().decode(), out

    def sky_call(nchan=3, vmin=-3., vmax=3., d=d, origin=origin, vo=None,
                 **f):
        f = dict(base, **f)
        out = np.full((3, len(d)), -7.)
        rc = lib.cmi_gpu_render_field_absorbing_sky_cube(
            h, *pointers(f), p(A._f64(origin)),
            None if vo is None else p(A._f64(vo)), len(d), p(A._f64(d)),
            nchan, vmin, vmax, p(out))
        return rc, lib.cmi_gpu_last_error().decode(), out

    def probe_call(nchan=3, point=0, **f):
        f = dict(base, **f)
        out = np.full((10, 3 + (2 + 3) * 4 + 3), -7.)
        view = A._f64(origin) if point else A._f64([theta, phi])
        rays = A._f64(d) if point else A._f64(np.zeros((10, 2)))
        rc = lib.cmi_gpu_absorbing_cube_probe(
            h, *pointers(f), nchan, -3., 3., point, p(view), None, 10,
            p(rays), 4, p(out))
        return rc, lib.cmi_gpu_last_error().decode(), out

    def hi_call(engine_handle=h, kind="cube", sigma=0., mode=0, spin=None,
                T_bg=0., nchan=3):
        out = np.full((3, NX, NY), -7.)
        ts = None if spin is None else p(A._f64(spin))
        if kind == "cube":
            rc = lib.cmi_gpu_render_hi_cube(
                engine_handle, theta, phi, NX, NY, p(A._f64(anchor)),
                p(A._f64(sides)), 1, nchan, -3., 3., sigma, mode, ts, 1, T_bg,
                p(out))
        elif kind == "sky":
            rc = lib.cmi_gpu_render_hi_sky_cube(
                engine_handle, p(A._f64(origin)), None, len(d), p(A._f64(d)),
                nchan, -3., 3., sigma, mode, ts, 1, T_bg, p(out))
        elif kind == "map":
            rc = lib.cmi_gpu_render_hi_sky_map_cube(
                engine_handle, p(A._f64(origin)),
                p(A._f64(E.IDENTITY_FRAME).reshape(9)), -1., 2., -0.5, 1., 8,
                6, None, nchan, -3., 3., sigma, mode, ts, 1, T_bg, p(out))
        else:
            # (five arrays of a cell each: a call that is not refused must
            # find room for what it writes)
            out = np.full((5, BOX.n), -7.)
            rc = lib.cmi_gpu_hi_coefficients(
                engine_handle, sigma, mode, ts, 1, *[p(row) for row in out])
        return rc, lib.cmi_gpu_last_error().decode(), out

    def bad(name, value, where=17):
        x = base[name].copy()
        x.reshape(-1)[where] = value
        return {name: x}

    far = base["sl"].copy()
    far[17] = 1e308
    near = base["sc"].copy()
    near[17] = -1e308
    cases = [
        (cube_call(nchan=0), "at least one velocity channel"),
        (sky_call(nchan=-3), "at least one velocity channel"),
        (cube_call(vmin=3., vmax=3.), "velocity range must be finite"),
        (sky_call(vmax=np.inf), "velocity range must be finite"),
        (cube_call(**bad("a", -1e-3)), "1 integrated line opacities"),
        (cube_call(**bad("a", np.nan)), "1 integrated line opacities"),
        (sky_call(**bad("a", np.inf)), "1 integrated line opacities"),
        # (finite, but not once divided by the channel width)
        (cube_call(vmin=0., vmax=3e-300, **bad("a", 1e10)),
         "1 integrated line opacities"),
        (cube_call(**bad("b", -1.)), "1 width(s)"),
        (sky_call(**bad("b", np.nan)), "1 width(s)"),
        (probe_call(**bad("b", np.inf)), "1 width(s)"),
        (cube_call(**bad("kc", -1e-3)), "1 continuum absorption"),
        (sky_call(**bad("kc", np.inf)), "1 continuum absorption"),
        (cube_call(**bad("sl", np.inf)), "1 line source function"),
        (sky_call(**bad("sl", np.nan)), "1 line source function"),
        (cube_call(**bad("sc", np.nan)), "1 continuum source function"),
        (sky_call(**bad("sc", -np.inf)), "1 continuum source function"),
        (cube_call(sl=far, sc=near), "1 continuum source function"),
        (cube_call(**bad("velocity", np.nan)), "1 velocity component(s)"),
        (sky_call(**bad("velocity", np.inf)), "1 velocity component(s)"),
        (cube_call(**bad("background", np.nan, 1)), "background of channel 1"),
        (sky_call(**bad("background", -np.inf, 0)), "background of channel 0"),
        (probe_call(**bad("background", np.nan, 2)),
         "background of channel 2"),
        (cube_call(kc=None), "come together or not at all"),
        (sky_call(sc=None), "come together or not at all"),
        (cube_call(a=None), "null argument"),
        (sky_call(b=None), "null argument"),
        (probe_call(sl=None), "null argument"),
        (probe_call(nchan=2000), "between 1 and 1024 channels"),
        (cube_call(nx=0), "between 1 and 2^28 pixels"),
        (cube_call(theta=np.nan), "view angles must be finite"),
        (cube_call(s=9), "supersampling must be 1..8"),
        (sky_call(d=2. * d), "not a unit vector"),
        (sky_call(origin=(0., np.nan, 0.)), "origin is not finite"),
        (sky_call(vo=(0., np.inf, 0.)), "observer's velocity is not finite"),
        (hi_call(sigma=-1.), "turbulent velocity dispersion"),
        (hi_call(kind="sky", mode=3), "no spin temperature mode 3"),
        (hi_call(kind="map", mode=1), "needs a spin temperature"),
        (hi_call(mode=1, spin=[0.]), "spin temperature must be positive"),
        (hi_call(kind="coefficients", mode=1, spin=[np.inf]),
         "spin temperature must be positive"),
        (hi_call(mode=2, spin=bad("a", np.nan)["a"]),
         "1 spin temperature(s) are not finite"),
        # finite cells whose coefficients overflow: a = C n_HI / T_s = 5.5e-12 /
        # 1e-322 = inf
        (hi_call(mode=1, spin=[1e-322]), "21-cm coefficient that is not"),
        (hi_call(kind="sky", mode=1, spin=[1e-322]),
         "21-cm coefficient that is not"),
        (hi_call(kind="coefficients", mode=1, spin=[1e-322]),
         "21-cm coefficient that is not"),
        (hi_call(kind="map", mode=2,
                 spin=np.where(np.arange(BOX.n) == 17, 1e-322, 50.)),
         "1 cell(s) have a 21-cm coefficient that is not"),
        (hi_call(T_bg=-1.), "background temperature must be >= 0"),
        (hi_call(kind="sky", T_bg=np.nan),
         "background temperature must be >= 0"),
        (hi_call(nchan=0), "at least one velocity channel"),
    ]
    for (rc, message, out), word in cases:
        assert rc == EINVAL and word in message, (rc, message, word)
        assert (out == -7.).all(), word
    # the limit of the cube calls: nchan * npixel <= 2^28
    rc, message, out = cube_call(nchan=(1 << 28) // (NX * NY) + 1,
                                 background=None)
    assert rc == EINVAL and "2^28" in message and (out == -7.).all()
    rc, message, out = hi_call(kind="map", nchan=(1 << 28) // 48 + 1)
    assert rc == EINVAL and "2^28" in message and (out == -7.).all()
    # the H I calls need cells
    fresh = E.GpuEngine(tuple(int(n) for n in BOX.ncell), tuple(BOX.anchor),
                        tuple(BOX.sides), (0, 0, 0), device=0)
    for kind in ("cube", "sky", "map", "coefficients"):
        rc, message, out = hi_call(engine_handle=fresh._h, kind=kind)
        assert rc == ESTATE and "cell data must be set first" in message
        assert (out == -7.).all()
    fresh.close()
    periodic = E.GpuEngine((4, 4, 4), (0., 0., 0.), (1., 1., 1.), (1, 0, 0),
                           device=0)
    one = np.ones(64)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.render_field_absorbing_cube(one, one, one, 0., 0., 4, 4,
                                             (0., 0.), (1., 1.), 3, -1., 1.)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.render_field_absorbing_sky_cube(one, one, one,
                                                 (0.5, 0.5, 0.5), d, 3, -1.,
                                                 1.)
    periodic.close()
    # a block of a decomposed grid: every call of the section, the
    # coefficients and the probe in both forms included, with cells set so
    # that nothing else stands in the way
    block = E.GpuEngine((8, 4, 4), (0., 0., 0.), (1., 1., 1.), (0, 0, 0),
                        device=0, sub_offset=(4, 0, 0), sub_ncell=(4, 4, 4))
    block.upload_cells(np.full(64, 1e8), np.full(64, 100.),
                       np.ones((E.NION, 64)))
    bh = block._h
    f64 = [p(np.ones(64)) for _ in range(3)] + [None] * 4
    image = [p(A._f64((-1., -1.))), p(A._f64((2., 2.)))]
    view, inside = A._f64([0.3, 0.2]), A._f64((0.7, 0.5, 0.5))
    rays2, rays3 = np.zeros((10, 2)), A._f64(d)
    frame = A._f64(E.IDENTITY_FRAME).reshape(9)
    axis = (3, -3., 3.)
    hi = (0., 0, None, 1)
    block_calls = {
        "render_field_absorbing_cube": lambda out: (
            lib.cmi_gpu_render_field_absorbing_cube(
                bh, *f64, 0.3, 0.2, 4, 4, *image, 1, *axis, p(out))),
        "render_field_absorbing_sky_cube": lambda out: (
            lib.cmi_gpu_render_field_absorbing_sky_cube(
                bh, *f64, p(inside), None, 10, p(rays3), *axis, p(out))),
        "absorbing_cube_probe": lambda out: (
            lib.cmi_gpu_absorbing_cube_probe(
                bh, *f64, *axis, 0, p(view), None, 10, p(rays2), 4, p(out))),
        "absorbing_cube_probe point": lambda out: (
            lib.cmi_gpu_absorbing_cube_probe(
                bh, *f64, *axis, 1, p(inside), None, 10, p(rays3), 4,
                p(out))),
        "render_hi_cube": lambda out: lib.cmi_gpu_render_hi_cube(
            bh, 0.3, 0.2, 4, 4, *image, 1, *axis, *hi, 0., p(out)),
        "render_hi_sky_cube": lambda out: lib.cmi_gpu_render_hi_sky_cube(
            bh, p(inside), None, 10, p(rays3), *axis, *hi, 0., p(out)),
        "render_hi_sky_map_cube": lambda out: (
            lib.cmi_gpu_render_hi_sky_map_cube(
                bh, p(inside), p(frame), -1., 2., -0.5, 1., 8, 6, None, *axis,
                *hi, 0., p(out))),
        "hi_coefficients": lambda out: lib.cmi_gpu_hi_coefficients(
            bh, *hi, p(out), p(out[64:]), p(out[128:]), p(out[192:]),
            p(out[256:])),
    }
    for name, call in block_calls.items():
        out = np.full(512, -7.)
        rc = call(out)
        message = lib.cmi_gpu_last_error().decode()
        assert rc == ESTATE and "decomposed" in message, (name, rc, message)
        # (the map call is refused by the ray-list call it makes, as
        # render_line_sky_map_cube is)
        says = name.split()[0].replace("sky_map_cube", "sky_cube")
        assert message.startswith(says + ":"), message
        assert (out == -7.).all(), name
    block.close()
    # the engine is still usable
    rc, message, out = cube_call()
    assert rc == 0 and not (out == -7.).any()
    rc, message, out = sky_call()
    assert rc == 0 and not (out == -7.).any()
