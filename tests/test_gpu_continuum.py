"""Continuum images on the device (include/cmi_gpu.h, "continuum images";
DESIGN.md 4.15) through the C ABI: the contract's exact identities, the
independence of a channel from its block and its chunk, parity with the CPU
restatement (tests/support/continuum_reference.c, checked on its own in
test_continuum_host.py) within a derived bound, the grey limit against the
line images and sky maps, the probe, the free-free coefficients against their
numpy form, the physics of a uniform H II region, and the refusals."""
import numpy as np
import pytest

import continuum_lib as K
import line_image_lib as L

pytestmark = pytest.mark.gpu

EPS = K.EPS
BOX, NX, NY, VIEWS = K.BOX, K.NX, K.NY, K.VIEWS
FB = K.channel_block()
EINVAL, ESTATE = 1, 3  # include/cmi_gpu.h


@pytest.fixture(scope="module")
def eng():
    from cmacionize_amd import GpuEngine
    engine = GpuEngine(tuple(int(n) for n in BOX.ncell), tuple(BOX.anchor),
                       tuple(BOX.sides), (0, 0, 0), device=0)
    yield engine
    engine.close()


@pytest.fixture(scope="module")
def channels():
    """2 FB + 3 random channels, shared and left unchanged"""
    kappa, S, bg = K.random_channels(BOX, 2 * FB + 3, 101)
    for a in (kappa, S, bg):
        a.setflags(write=False)
    return kappa, S, bg


def rectangle(view):
    return K.image_rectangle(BOX, *VIEWS[view])


# ------------------------------------------------------------ 1 identities --

def test_exact_identities(eng, channels):
    """kappa == 0 gives bg in every pixel and channel, rays that miss
    included; S_f == bg_f with random kappa gives bg (parallel camera); a
    second call gives the bits of the first"""
    kappa, S, bg = (a[:FB + 1] for a in channels)
    for view, (theta, phi) in enumerate(VIEWS):
        anchor, sides = rectangle(view)
        flat = np.broadcast_to(bg[:, None, None], (len(bg), NX, NY))
        got = eng.render_field_continuum_images(
            np.zeros_like(kappa), S, theta, phi, NX, NY, anchor, sides,
            background=bg)
        assert np.array_equal(got, flat), (theta, phi)
        source = bg[:, None] * np.ones(BOX.n)
        got = eng.render_field_continuum_images(
            kappa, source, theta, phi, NX, NY, anchor, sides, background=bg)
        assert np.array_equal(got, flat), (theta, phi)
        for s in (1, 3):
            a = eng.render_field_continuum_images(
                kappa, S, theta, phi, NX, NY, anchor, sides, s, background=bg)
            b = eng.render_field_continuum_images(
                kappa, S, theta, phi, NX, NY, anchor, sides, s, background=bg)
            assert np.array_equal(a, b) and not np.isnan(a).any()
            # (an axis-aligned view has one value per column of cells)
            assert len(np.unique(a[0])) > 50
    d = K.sky_directions()
    for origin in K.sky_origins(BOX):
        got = eng.render_field_continuum_sky(np.zeros_like(kappa), S, origin,
                                             d, background=bg)
        assert np.array_equal(got, np.broadcast_to(bg[:, None], got.shape))
        a = eng.render_field_continuum_sky(kappa, S, origin, d, background=bg)
        b = eng.render_field_continuum_sky(kappa, S, origin, d, background=bg)
        assert np.array_equal(a, b) and not np.isnan(a).any()
    # without a background: zero
    got = eng.render_field_continuum_images(
        np.zeros_like(kappa), S, 0.7, 0.3, NX, NY, *rectangle(3))
    assert not got.any()


# ------------------------------------------------- 2 block independence --

def test_channel_block_independence(eng, channels):
    """a channel's image and sky are the same bits whether nf is 1, FB - 1,
    FB, FB + 1 or 2 FB + 3, wherever it sits in the list, for every block
    width, and across the chunk boundary of the sample rows and rays"""
    kappa, S, bg = channels
    nall = len(kappa)
    theta, phi = VIEWS[3]
    anchor, sides = rectangle(3)
    origin = K.sky_origins(BOX)[0]
    d = K.sky_directions()

    def both(order, s=3):
        order = list(order)
        img = eng.render_field_continuum_images(
            kappa[order], S[order], theta, phi, NX, NY, anchor, sides, s,
            background=bg[order])
        sk = eng.render_field_continuum_sky(kappa[order], S[order], origin, d,
                                            background=bg[order])
        return img, sk

    full_img, full_sky = both(range(nall))
    alone = [both([c]) for c in range(nall)]
    for c in range(nall):
        assert np.array_equal(alone[c][0][0], full_img[c]), c
        assert np.array_equal(alone[c][1][0], full_sky[c]), c
    rng = np.random.default_rng(3)
    for nf in sorted({1, FB - 1, FB, FB + 1, 2 * FB + 3}):
        order = rng.permutation(nall)[:nf]
        img, sk = both(order)
        assert np.array_equal(img, full_img[order]), nf
        assert np.array_equal(sk, full_sky[order]), nf
    try:
        for width in (4, 8, 16):
            eng.set_tuning(continuum_channel_block=width)
            img, sk = both(range(nall))
            assert np.array_equal(img, full_img), width
            assert np.array_equal(sk, full_sky), width
        eng.set_tuning(continuum_channel_block=FB)
        # 3 * NY * 3 = 153 sample rays per pixel row: chunks of 2 rows of
        # pixels (23 rows: a last chunk of one), and of 1; 100 rays per
        # launch (500 rays: full chunks), and 64 and 333 (a partial last)
        for launch in (2 * 153, 1, 100, 64, 333):
            eng.set_tuning(continuum_launch_rays=launch)
            img, sk = both(range(nall))
            assert np.array_equal(img, full_img), launch
            assert np.array_equal(sk, full_sky), launch
    finally:
        eng.set_tuning(continuum_channel_block=FB, continuum_launch_rays=0)


# --------------------------------------------------------------- 3 parity --

@pytest.mark.parametrize("s", [1, 3])
def test_parity_with_the_restatement_parallel(eng, channels, s):
    """|gpu - cpu| <= march_bound (continuum_lib has the derivation: the
    rounding of the contract's operations and the 2 ulps between the device's
    and glibc's expm1 per crossing, times the crossings of the longest ray,
    scaled by max(|S|, |bg|)), per channel, in all six views; tau per cell
    spans 1e-12 to 50 with a tenth of the cells at exactly 0"""
    kappa, S, bg = (a[:FB + 1] for a in channels)
    tau = kappa * BOX.cellside.mean()
    assert (tau == 0.).mean() > 0.05 and tau.max() > 40.
    assert tau[tau > 0.].min() < 1e-11
    worst = 0.
    for view, (theta, phi) in enumerate(VIEWS):
        anchor, sides = rectangle(view)
        want = K.images(BOX, kappa, S, theta, phi, NX, NY, anchor, sides, s,
                        background=bg)
        steps = K.longest_ray
        got = eng.render_field_continuum_images(
            kappa, S, theta, phi, NX, NY, anchor, sides, s, background=bg)
        assert got.shape == want.shape and not np.isnan(got).any()
        for f in range(len(kappa)):
            bound = K.march_bound(steps, S[f], bg[f:f + 1], supersample=s)
            ratio = np.abs(got[f] - want[f]).max() / bound
            worst = max(worst, ratio)
            assert ratio <= 1., (theta, phi, f, ratio)
        print("parallel s", s, "view", theta, phi, "steps", steps)
    print("parallel s %d: largest |gpu - cpu| / bound %.4f" % (s, worst))


def test_parity_with_the_restatement_point(eng, channels):
    """the same for rays from a point: an origin inside a cell, one on a cell
    wall, one outside; 500 directions with the axis-parallel ones"""
    kappa, S, bg = (a[:FB + 1] for a in channels)
    worst = 0.
    for origin in K.sky_origins(BOX):
        # (half of the random directions aim at the box: the observer
        # outside sees it in more than a handful of rays)
        d = K.sky_directions(box=BOX, origin=origin)
        assert len(d) == 500
        want = K.sky(BOX, kappa, S, origin, d, background=bg)
        steps = K.longest_ray
        got = eng.render_field_continuum_sky(kappa, S, origin, d,
                                             background=bg)
        assert got.shape == want.shape and not np.isnan(got).any()
        assert (want != bg[:, None]).mean() > 0.4
        for f in range(len(kappa)):
            bound = K.march_bound(steps, S[f], bg[f:f + 1], point=True)
            ratio = np.abs(got[f] - want[f]).max() / bound
            worst = max(worst, ratio)
            assert ratio <= 1., (origin, f, ratio)
    print("point: largest |gpu - cpu| / bound %.4f" % worst)


# ----------------------------------------------------------- 4 grey limit --

# Device against device: the images march I = I att + s emit with att =
# exp(-dtau), emit = -expm1(-dtau) and s = (4 pi field / (4 pi)) / k; the
# continuum I = I + em (I - S) with S = field / k. Per crossing, in units of
# M EPS (M = max S): att against 1 + em, 1 ulp of exp, 1 ulp of expm1 and the
# rounding of the sum, 5; s against S, three more roundings than S has and
# its own, 4; the roundings of the images' step, 3, and of the continuum's,
# 5: 17. Rays from a point: 8 for T (5 and the three roundings of the two
# forms) through the telescoping sum of continuum_lib, 4 for s, 3 + 3
# roundings: 18.
GREY_PARALLEL, GREY_POINT = 17., 18.


def test_grey_limit(eng):
    rng = np.random.default_rng(77)
    nf = 3
    k = np.exp(rng.uniform(np.log(1e-6), np.log(50.), BOX.n)) / \
        BOX.cellside.mean()
    field = 10. ** rng.uniform(-2., 1., (nf, BOX.n))
    kappa = np.broadcast_to(k, (nf, BOX.n))
    S = field / k
    M = S.max(axis=1)
    worst = 0.
    for view, (theta, phi) in enumerate(VIEWS):
        anchor, sides = rectangle(view)
        for s in (1, 3):
            want = eng.render_field_images(4. * np.pi * field, theta, phi, NX,
                                           NY, anchor, sides, s, extinction=k)
            got = eng.render_field_continuum_images(kappa, S, theta, phi, NX,
                                                    NY, anchor, sides, s)
            K.images(BOX, kappa[:1], S[:1], theta, phi, NX, NY, anchor, sides,
                     s)
            bound = (GREY_PARALLEL * K.longest_ray + 2 * (s * s + 1)) * M * EPS
            ratio = (np.abs(got - want).max(axis=(1, 2)) / bound).max()
            worst = max(worst, ratio)
            assert ratio <= 1., (theta, phi, s, ratio)
            assert want.max() > 0.
    for origin in K.sky_origins(BOX):
        d = K.sky_directions(box=BOX, origin=origin)
        want = eng.render_field_sky(4. * np.pi * field, origin, d,
                                    extinction=k)
        got = eng.render_field_continuum_sky(kappa, S, origin, d)
        K.sky(BOX, kappa[:1], S[:1], origin, d)
        bound = (GREY_POINT * K.longest_ray + 4.) * M * EPS
        ratio = (np.abs(got - want).max(axis=1) / bound).max()
        worst = max(worst, ratio)
        assert ratio <= 1., (origin, ratio)
    print("grey limit: largest difference / bound %.3g" % worst)


# ---------------------------------------------------------------- 5 probe --

def test_probe_traces(eng, channels):
    """the (cell, ds) lists equal the restatement's exactly, the running I_f
    agrees within the bound of its step count, I_end is the render call's"""
    kappa, S, bg = (a[:3] for a in channels)
    m = 40
    theta, phi = VIEWS[4]
    anchor, sides = rectangle(4)
    xy = L.sample_coordinates(NX, NY, anchor, sides).reshape(-1, 2)
    cases = [(dict(theta=theta, phi=phi), xy, False)]
    for origin in K.sky_origins(BOX):
        cases.append((dict(origin=origin),
                      K.sky_directions(box=BOX, origin=origin), True))
    for where, rays, point in cases:
        got = eng.continuum_probe(kappa, S, rays, m, background=bg, **where)
        want = K.probe(BOX, kappa, S, rays, m, background=bg, **where)
        gt, gsteps, gcells, gds, gI, gend = K.split_probe(got, 3, m)
        wt, wsteps, wcells, wds, wI, wend = K.split_probe(want, 3, m)
        assert np.array_equal(gt, wt, equal_nan=True)
        assert np.array_equal(gsteps, wsteps) and gsteps.max() <= m
        assert (gsteps > 10).any()
        if not point:
            assert (gsteps == 0).any()      # the margin: rays that miss
        assert np.array_equal(gcells, wcells) and np.array_equal(gds, wds)
        step = np.arange(1, m + 1)
        for f in range(3):
            per = K.STEP_EPS_POINT if point else K.STEP_EPS_PARALLEL
            scale = max(S[f].max(), bg[f]) * EPS
            assert (np.abs(gI[:, f] - wI[:, f]) <= per * step * scale).all()
            assert (np.abs(gend[:, f] - wend[:, f]) <=
                    (per * np.maximum(gsteps, 1) + 4.) * scale).all()
        if point:
            render = eng.render_field_continuum_sky(
                kappa, S, where["origin"], rays, background=bg)
        else:
            render = eng.render_field_continuum_images(
                kappa, S, theta, phi, NX, NY, anchor, sides,
                background=bg).reshape(3, -1)
        assert np.array_equal(gend.T, render)


# --------------------------------------------------------- 6 coefficients --

def lattice():
    """cells: vacuum, fully neutral, T = 0, and T from 500 to 3e4 K at three
    densities and three ionization states; padded to the box with vacuum"""
    rows = [(0., 1e4, 0., 0.), (1e8, 1e4, 1., 1.), (1e8, 0., 0., 0.)]
    for T in (500., 1e3, 3e3, 7.5e3, 1e4, 1.7e4, 3e4):
        for n in (1e6, 1e8, 3.3e10):
            for xH, xHe in ((0., 0.), (1e-3, 0.4), (0.5, 1.)):
                rows.append((n, T, xH, xHe))
    rows = np.array(rows).T
    cells = np.zeros((4, BOX.n))
    cells[1] = 1e4
    cells[:, :rows.shape[1]] = rows
    return cells, rows.shape[1]


@pytest.mark.parametrize("helium", [0.1, 0.])
def test_free_free_coefficients(eng, helium):
    """against the numpy form. The special cells give exactly (0, 0). For the
    others, in units of EPS = 2^-53 (1 ulp <= 2 EPS) with device and host
    log, exp, pow and expm1 each documented within 1 ulp, 4 EPS between the
    two: S = A / expm1(x), 4 and the division's rounding on either side, 6.
    y = (nu / 1e9) pow(T / 1e4, -1.5) differs by 4 + 2; log y by that and 4
    |log y|; the exponent a = 5.96 - c log y by c times that and two
    roundings of at most |a| + 5.96 on either side; exp(a) relatively by that
    and 4; g = log(exp(a) + e) >= 1 by no more, and 2 + 4 |g| / |g|; j has
    six more operations, 12, and exp(-x), 4; kappa = j / S one more, 2, and
    S's 6."""
    from cmacionize_amd import engine as E
    cells, used = lattice()
    n, T, xH, xHe = cells
    x = np.zeros((E.NION, BOX.n))
    x[0], x[1] = xH, xHe
    eng.set_abundances([helium, 0., 0., 0., 0., 0.])
    eng.upload_cells(n, T, x)
    nu = 10. ** np.linspace(7., 12., 2 * FB + 1)
    kappa, S = eng.free_free_coefficients(nu)
    wk, ws = K.free_free(n, T, xH, xHe, helium, nu)
    assert kappa.shape == S.shape == (len(nu), BOX.n)
    special = np.ones(BOX.n, dtype=bool)
    special[3:used] = False
    if helium == 0.:
        special |= xH == 1.     # helium off: hydrogen neutral, no electrons
    assert not kappa[:, special].any() and not S[:, special].any()
    assert not wk[:, special].any() and not ws[:, special].any()
    live = ~special
    assert (kappa[:, live] > 0.).all() and (S[:, live] > 0.).all()
    assert np.isfinite(kappa).all() and np.isfinite(S).all()
    y = (nu[:, None] / 1e9) * np.power(T[live] / 1e4, -1.5)[None, :]
    c = np.sqrt(3.) / np.pi
    a = 5.960 - c * np.log(y)
    d_logy = 6. + 4. * np.abs(np.log(y))
    d_a = c * d_logy + 4. * (np.abs(a) + 5.960)
    d_g = (d_a + 4.) + 2. + 4.
    bound_k = (d_g + 12. + 4. + 2. + 6.) * EPS
    rs = np.abs(S[:, live] / ws[:, live] - 1.)
    rk = np.abs(kappa[:, live] / wk[:, live] - 1.)
    print("helium %g: S within %.2f ulp (6 EPS = 3 ulp allowed), kappa within "
          "%.2f ulp, %.3f of its bound (%.0f to %.0f ulp)" %
          (helium, rs.max() / (2 * EPS), rk.max() / (2 * EPS),
           (rk / bound_k).max(), bound_k.min() / (2 * EPS),
           bound_k.max() / (2 * EPS)))
    assert (rs <= 6. * EPS).all()
    assert (rk <= bound_k).all()


# -------------------------------------------------------------- 7 physics --

def test_uniform_h_ii_region(eng):
    """a uniform ionized box seen along z: I_nu = B_nu(T) (1 - exp(-kappa L))
    from thin to tau > 40, the coefficients' and the march's bounds together;
    at the thick end the brightness temperature is T, and a background shines
    through only where the gas is thin. (The test box is metres across: the
    density is what makes it thick at 3 MHz, not what a nebula has.)"""
    from cmacionize_amd import engine as E
    T, n, helium = 8000., 1.e16, 0.1
    x = np.zeros((E.NION, BOX.n))
    eng.set_abundances([helium, 0., 0., 0., 0., 0.])
    eng.upload_cells(np.full(BOX.n, n), np.full(BOX.n, T), x)
    nu = 10. ** np.linspace(6.5, 11., 12)
    anchor, sides = K.image_rectangle(BOX, 0., 0.)
    img = eng.render_continuum_images(nu, 0., 0., NX, NY, anchor, sides)
    assert img.shape == (len(nu), NX, NY)
    xy = L.sample_coordinates(NX, NY, anchor, sides).reshape(-1, 2)
    hit = (L.chords(BOX, 0., 0., xy) > 0.).reshape(NX, NY)
    assert 20 < hit.sum() < NX * NY - 20 and not img[:, ~hit].any()
    wk, ws = K.free_free([n], [T], [0.], [0.], helium, nu)
    depth, cells = BOX.sides[2], int(BOX.ncell[2])
    tau = wk[:, 0] * depth
    assert tau[0] > 40. and tau[-1] < 1e-3
    want = ws[:, 0] * -np.expm1(-tau)
    # relative: kappa's 60 ulp and S's 3 (test_free_free_coefficients), the
    # march's 18 EPS per cell, and the sum of the cells' tau
    allowed = (120. + 6. + (K.STEP_EPS_PARALLEL + 2.) * cells + 4.) * EPS
    err = np.abs(img[:, hit] / want[:, None] - 1.).max()
    print("uniform H II region: worst relative error %.3g, allowed %.3g" %
          (err, allowed))
    assert err <= allowed
    Tb = E.brightness_temperature(img, nu)[:, hit]
    # Rayleigh-Jeans at 3 MHz: h nu / (2 k T) = 1e-8
    assert np.abs(Tb[0] / T - 1.).max() < 1e-7
    assert (Tb[-1] < 1e-2 * T).all()
    index = E.continuum_spectral_index(img, nu)[:, hit]
    assert np.abs(index[0] - 2.).max() < 1e-3
    assert (-0.2 < index[-1]).all() and (index[-1] < -0.05).all()
    bg = E.planck_function(nu, 2.725)
    lit = eng.render_continuum_images(nu, 0., 0., NX, NY, anchor, sides,
                                      background=bg)
    assert np.array_equal(lit[:, ~hit],
                          np.broadcast_to(bg[:, None], (len(nu),
                                                        (~hit).sum())))
    assert np.array_equal(lit[0], np.where(hit, img[0], bg[0]))  # thick
    # the sky from inside, and the map: the ray-list call on its directions
    origin = BOX.anchor + 0.5 * BOX.sides
    d, _ = E.sky_map_directions(16, 9)
    sky = eng.render_continuum_sky(nu, origin, d.reshape(-1, 3),
                                   background=bg)
    maps = eng.render_continuum_sky_map(nu, origin, 16, 9, background=bg)
    assert np.array_equal(maps.reshape(len(nu), -1), sky)
    assert np.abs(E.brightness_temperature(sky, nu)[0] / T - 1.).max() < 1e-7


# ------------------------------------------------------------ 8 refusals --

def test_refusals(eng, channels):
    from cmacionize_amd import engine as E
    kappa, S, bg = (a[:2].copy() for a in channels)
    theta, phi = VIEWS[3]
    anchor, sides = rectangle(3)
    d = K.sky_directions()[:10]
    origin = K.sky_origins(BOX)[0]
    lib, h = eng._lib, eng._h
    nu = np.array([1e9, 5e9])

    def image_call(nf=2, kappa=kappa, S=S, bg=bg, nx=NX, theta=theta, s=1):
        out = np.full((2, NX, NY), -7.)
        rc = lib.cmi_gpu_render_field_continuum_images(
            h, nf, K._p(kappa), K._p(S), K._p(bg) if bg is not None else None,
            theta, phi, nx, NY, K._p(K._f64(anchor)), K._p(K._f64(sides)), s,
            K._p(out))
        return rc, lib.cmi_gpu_last_error().decode(), out

    def sky_call(nf=2, kappa=kappa, S=S, bg=bg, d=d, origin=origin):
        out = np.full((2, len(d)), -7.)
        rc = lib.cmi_gpu_render_field_continuum_sky(
            h, nf, K._p(kappa), K._p(S), K._p(bg), K._p(K._f64(origin)),
            len(d), K._p(K._f64(d)), K._p(out))
        return rc, lib.cmi_gpu_last_error().decode(), out

    def free_call(nu=nu, engine_handle=h, kind="images"):
        out = np.full((2, NX, NY), -7.)
        v = K._f64(nu)
        if kind == "images":
            rc = lib.cmi_gpu_render_continuum_images(
                engine_handle, len(v), K._p(v), None, theta, phi, NX, NY,
                K._p(K._f64(anchor)), K._p(K._f64(sides)), 1, K._p(out))
        elif kind == "sky":
            rc = lib.cmi_gpu_render_continuum_sky(
                engine_handle, len(v), K._p(v), None, K._p(K._f64(origin)),
                len(d), K._p(K._f64(d)), K._p(out))
        else:
            rc = lib.cmi_gpu_free_free_coefficients(
                engine_handle, len(v), K._p(v), K._p(out), K._p(out))
        return rc, lib.cmi_gpu_last_error().decode(), out

    def map_call(nlon=8, lon=(-1., 2.), lat=(-0.5, 1.),
                 frame=E.IDENTITY_FRAME, nu=nu):
        out = np.full((2, 8, 6), -7.)
        v = K._f64(nu)
        rc = lib.cmi_gpu_render_continuum_sky_map(
            h, len(v), K._p(v), None, K._p(K._f64(origin)), nlon, 6,
            K._p(K._f64(lon)), K._p(K._f64(lat)),
            K._p(K._f64(frame).reshape(9)), K._p(out))
        return rc, lib.cmi_gpu_last_error().decode(), out

    def bad(a, value, where=(1, 17)):
        a = a.copy()
        a[where] = value
        return a

    cases = [
        (image_call(nf=0), "at least one channel"),
        (sky_call(nf=-3), "at least one channel"),
        (image_call(kappa=bad(kappa, -1e-3)), "1 absorption coefficient(s)"),
        (image_call(kappa=bad(kappa, np.nan)), "1 absorption coefficient(s)"),
        (sky_call(kappa=bad(kappa, np.inf)), "1 absorption coefficient(s)"),
        (image_call(S=bad(S, np.inf)), "1 source function value(s)"),
        (sky_call(S=bad(S, np.nan)), "1 source function value(s)"),
        (image_call(bg=bad(bg, np.nan, 1)), "background of channel 1"),
        (sky_call(bg=bad(bg, -np.inf, 0)), "background of channel 0"),
        (image_call(nx=0), "between 1 and 2^28 pixels"),
        (image_call(theta=np.nan), "view angles must be finite"),
        (image_call(s=9), "supersampling must be 1..8"),
        (sky_call(d=2. * d), "not a unit vector"),
        (sky_call(origin=(0., np.nan, 0.)), "origin is not finite"),
        (free_call(nu=[1e9, 0.]), "frequency 1 is not finite and positive"),
        (free_call(nu=[-1e9, 1e9], kind="sky"),
         "frequency 0 is not finite and positive"),
        (free_call(nu=[np.inf, 1e9], kind="coefficients"),
         "frequency 0 is not finite and positive"),
        # the map call: what render_line_sky_map refuses for its map
        (map_call(nlon=0), "between 1 and 2^28 pixels"),
        (map_call(lon=(2., -1.)), "longitude range must be finite and"),
        (map_call(lat=(-0.5, 1.7)), "latitude range must be increasing"),
        (map_call(frame=((1., 0., 0.), (0., 1., 0.), (0., 0.1, 1.))),
         "frame is not orthonormal"),
        (map_call(nu=[1e9, np.nan]), "frequency 1 is not finite and positive"),
    ]
    for (rc, message, out), word in cases:
        assert rc == EINVAL and word in message, (rc, message, word)
        assert (out == -7.).all(), word
    # the limit the cube calls put on their channels: nf * npixel <= 2^28
    rc, message, out = image_call(nf=(1 << 28) // (NX * NY) + 1)
    assert rc == EINVAL and "2^28" in message and (out == -7.).all()
    # the free-free calls need cells
    fresh = E.GpuEngine(tuple(int(n) for n in BOX.ncell), tuple(BOX.anchor),
                        tuple(BOX.sides), (0, 0, 0), device=0)
    for kind in ("images", "sky", "coefficients"):
        rc, message, out = free_call(engine_handle=fresh._h, kind=kind)
        assert rc == ESTATE and "cell data must be set first" in message
        assert (out == -7.).all()
    fresh.close()
    periodic = E.GpuEngine((4, 4, 4), (0., 0., 0.), (1., 1., 1.), (1, 0, 0),
                           device=0)
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.render_field_continuum_images(
            np.ones((1, 64)), np.ones((1, 64)), 0., 0., 4, 4, (0., 0.),
            (1., 1.))
    with pytest.raises(E.EngineError, match="periodic"):
        periodic.render_field_continuum_sky(
            np.ones((1, 64)), np.ones((1, 64)), (0.5, 0.5, 0.5), d)
    periodic.close()
    with pytest.raises(E.EngineError, match="4, 8 or 16"):
        eng.set_tuning(continuum_channel_block=5)
    # the engine is still usable
    rc, message, out = image_call()
    assert rc == 0 and not (out == -7.).any()
    rc, message, out = map_call()
    assert rc == 0 and not (out == -7.).any()
