"""Absorption spectra on the device (include/cmi_gpu.h, "absorption spectra";
DESIGN.md 4.19) through the C ABI: the contract's exact identities (the tuning
keys, the order of the rays, L = inf, the probe's geometry, sub-axes, the
Galilean shift), the identities within derived bounds (the sum rule, the
column density, the absorbing sky cube, additivity of the cut, parity with
the CPU restatement tests/support/absorption_reference.c), a slab against the
formula, the H I line's Voigt parameter, the refusals and the probe."""
import numpy as np
import pytest

import absorption_lib as AB

pytestmark = pytest.mark.gpu

EPS = AB.EPS
BOX, DV = AB.BOX, AB.DV
S, G = AB.LINE_S, AB.LINE_G
EINVAL, ESTATE = 1, 3  # include/cmi_gpu.h
MAX_CELLS = 40


@pytest.fixture(scope="module")
def eng():
    from cmacionize_amd import GpuEngine
    engine = GpuEngine(tuple(int(n) for n in BOX.ncell), tuple(BOX.anchor),
                       tuple(BOX.sides), (0, 0, 0), device=0)
    yield engine
    engine.close()


@pytest.fixture(scope="module")
def lines():
    """random lines, shared and left unchanged"""
    n, b, vel = AB.random_lines(BOX, 211)
    o, d, ln = AB.sightlines(BOX)
    for x in (n, b, vel, o, d, ln):
        x.setflags(write=False)
    return dict(n=n, b=b, velocity=vel, o=o, d=d, L=ln)


def gpu(eng, q, nchan, vmin, vmax, **more):
    f = dict(q, **more)
    return eng.render_field_absorption_spectra(
        f["n"], f["b"], f.get("S", S), f.get("g", G), f["o"], f["d"], nchan,
        vmin, vmax, lengths=f["L"], velocity=f["velocity"],
        observer_velocity=f.get("observer_velocity"))


@pytest.fixture(scope="module")
def reference(eng, lines):
    """device and restatement for every nchan of the tests, computed once"""
    out = {}
    for nchan in AB.NCHANS:
        nc, vmin, vmax = AB.axis_of(nchan)
        tau, N = gpu(eng, lines, nc, vmin, vmax)
        rtau, rN = AB.spectra(BOX, lines["n"], lines["b"], S, G, lines["o"],
                              lines["d"], lines["L"], nc, vmin, vmax,
                              velocity=lines["velocity"])
        for x in (tau, N, rtau, rN):
            x.setflags(write=False)
        out[nchan] = (tau, N, rtau, rN, AB.longest_ray)
    return out


# ------------------------------------------------------- exact identities --

def test_fields_are_what_the_issue_asks(lines):
    """the spread of the random cells (no device)"""
    ds = float(BOX.cellside.mean())
    depth = lines["n"] * ds * S[:, None] / DV
    assert depth[depth > 0.].min() < 1e-11 and depth.max() > 40.
    assert 0.05 < (lines["n"] == 0.).mean() < 0.15
    assert (lines["b"][0] == 0.).any() and (lines["b"][1:] > 0.).all()
    assert lines["b"].max() > 3.5 * DV
    a = G[:, None] / np.where(lines["b"] > 0., lines["b"], np.inf)
    assert G[0] == 0. and 1e-4 < np.median(a[1]) < 2e-3
    assert 0.01 < np.median(a[2]) < 0.2


@pytest.mark.parametrize("nchan", AB.NCHANS)
def test_tuning_changes_no_bit(eng, lines, reference, nchan):
    """the same bits for R in {1, 2, 4}, with and without the skips, with and
    without edge sharing, and on a second call"""
    nc, vmin, vmax = AB.axis_of(nchan)
    tau, N = reference[nchan][:2]
    assert tau.shape == (12, 3, nchan) and N.shape == (12, 3)
    assert not np.isnan(tau).any() and (tau >= 0.).all()
    if nchan > 1:
        assert len(np.unique(tau)) > 10 * nchan
    try:
        for rows in (1, 2, 4):
            for skips in (0, 1):
                for share in (0, 1):
                    eng.set_tuning(absorption_slab_rows=rows,
                                   absorption_skips=skips,
                                   absorption_edge_sharing=share)
                    t, n = gpu(eng, lines, nc, vmin, vmax)
                    assert np.array_equal(t, tau), (rows, skips, share)
                    assert np.array_equal(n, N), (rows, skips, share)
    finally:
        eng.set_tuning(absorption_slab_rows=0, absorption_skips=1,
                       absorption_edge_sharing=1)
    assert AB.default_rows() in (1, 2, 4)
    with pytest.raises(Exception, match="1, 2 or 4"):
        eng.set_tuning(absorption_slab_rows=3)


def test_skips_have_something_to_skip(eng, lines):
    """a band above most line centres: many cells are dark for its later
    slabs, and the bits are still those of the run without skips"""
    nc, vmin, vmax = 300, 3. * DV, 3. * DV + 300 * DV
    u = np.abs(lines["velocity"]).sum(axis=0)
    assert (u[None, :] + 6. * lines["b"] < vmin + 128 * DV).mean() > 0.5
    want = gpu(eng, lines, nc, vmin, vmax)
    try:
        eng.set_tuning(absorption_skips=0)
        got = gpu(eng, lines, nc, vmin, vmax)
    finally:
        eng.set_tuning(absorption_skips=1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[0][:, 0, 128:] == 0.).all()      # g == 0: nothing out there
    assert (want[0][:, 2, 128:].max(axis=1) > 0.).sum() >= 8   # wings


def test_ray_order_and_duplicates(eng, lines, reference):
    """permuting or duplicating rays permutes or duplicates the rows"""
    nc, vmin, vmax = AB.axis_of(65)
    tau, N = reference[65][:2]
    order = np.array([5, 0, 11, 3, 3, 8, 1, 10, 2, 7, 3, 9, 6, 4, 0])
    t, n = gpu(eng, lines, nc, vmin, vmax, o=lines["o"][order],
               d=lines["d"][order], L=lines["L"][order])
    assert np.array_equal(t, tau[order]) and np.array_equal(n, N[order])


def test_infinite_length_is_any_length_beyond_the_box(eng, lines, reference):
    """L = +inf equals any L >= t_out (t_out itself included)"""
    nc, vmin, vmax = AB.axis_of(65)
    o, d = lines["o"], lines["d"]
    inf = np.full(len(d), np.inf)
    want = gpu(eng, lines, nc, vmin, vmax, L=inf)
    t_out = np.array([eng.sky_probe(o[r], d[r:r + 1], 0)[0, 1]
                      for r in range(len(d))])
    hit = np.isfinite(t_out)
    assert hit.sum() >= 9
    for beyond in (t_out, t_out * (1. + 2. ** -50), t_out + 3.):
        got = gpu(eng, lines, nc, vmin, vmax,
                  L=np.where(hit, beyond, 1.))
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1])
    # and a finite length inside the box gives less
    assert (reference[65][1][[1, 2, 5]] < want[1][[1, 2, 5]]).all()


def test_probe_geometry_is_sky_probe(eng, lines):
    """with L = +inf the probe's (cell, ds) rows are sky_probe's, exactly"""
    o, d = lines["o"], lines["d"]
    nc, vmin, vmax = AB.axis_of(9)
    for r in range(len(d)):
        row = eng.absorption_probe(lines["n"][1], lines["b"][1], S[1], G[1],
                                   o[r], d[r], MAX_CELLS, nc, vmin, vmax,
                                   velocity=lines["velocity"])
        want = eng.sky_probe(o[r], d[r:r + 1], MAX_CELLS)[0]
        assert np.array_equal(row, want, equal_nan=True), r
        assert row[2] <= MAX_CELLS


def test_sub_axis(eng, lines, reference):
    """an axis that shares dv and starts on channel c0 of the long one
    reproduces those channels: DV = 2 and edges that are small integers, so
    that vmin + c * dv is exact on both axes"""
    tau = reference[300][0]
    _, vmin, _ = AB.axis_of(300)
    for c0, nsub in ((0, 64), (37, 65), (200, 100), (131, 1)):
        sub_min = vmin + c0 * DV
        got, _ = gpu(eng, lines, nsub, sub_min, sub_min + nsub * DV)
        assert np.array_equal(got, tau[:, :, c0:c0 + nsub]), (c0, nsub)


def test_velocity_shift_invariance(eng, lines):
    """rays along +z and -x exactly, velocities and edges in multiples of
    2^-3: shifting the axis by D and the observer by -D along the ray leaves
    every e - u, hence every bit, as it is"""
    rng = np.random.default_rng(47)
    vel = np.round(rng.uniform(-12., 12., (3, BOX.n)) * 8.) / 8.
    mid = BOX.anchor + BOX.cellside * np.array([5.5, 4.5, 3.5])
    D = 40.
    nchan, vmin, vmax = 70, -70., 70.
    for axis, sign in ((2, 1.), (0, -1.)):
        o = mid.copy()
        o[axis] = BOX.anchor[axis] - 1. if sign > 0 else \
            BOX.anchor[axis] + BOX.sides[axis] + 1.
        d = np.zeros(3)
        d[axis] = sign
        vo = np.zeros(3)
        vo[axis] = -D * sign      # u = (v - v_obs) . d = v . d + D
        q = dict(lines, o=o[None], d=d[None], L=np.array([np.inf]),
                 velocity=vel)
        one = gpu(eng, q, nchan, vmin, vmax)
        two = gpu(eng, q, nchan, vmin + D, vmax + D, observer_velocity=vo)
        assert np.array_equal(one[0], two[0]) and one[0].max() > 0.
        assert np.array_equal(one[1], two[1])


# ------------------------------------------- identities within a bound --

def test_sum_rule(eng, lines):
    """g == 0 and an axis that covers every line: sum_c tau_c dv == S N.
    Per crossing the f_c telescope: the E of the edges cancel in pairs but
    for the outermost, which are -1 and 1 exactly, and the roundings of the
    differences are EPS of each, 2 EPS of their sum; f / dv and A * are one
    rounding each; the sum into tau one per crossing; numpy's sum over the
    channels at most nchan; N's sum one per crossing; nds is shared; S * N
    and * dv one each: a relative (2 crossings + nchan + 6) EPS."""
    nchan = 128
    nc, vmin, vmax = AB.axis_of(nchan)
    u = np.abs(lines["velocity"]).sum(axis=0)
    assert (u[None, :] + 6. * lines["b"]).max() < vmax
    zero = np.zeros(3)
    tau, N = gpu(eng, lines, nc, vmin, vmax, g=zero)
    lhs = tau.sum(axis=2) * DV
    rhs = S[None, :] * N
    bound = (2 * MAX_CELLS + nchan + 6) * EPS * rhs
    ratio = np.abs(lhs - rhs) / np.where(bound > 0., bound, 1.)
    print("sum rule: |sum tau dv - S N| / bound = %.3f" % ratio.max())
    assert (N > 0.).sum() >= 24 and ratio.max() <= 1.
    assert np.array_equal(lhs[N == 0.], rhs[N == 0.])


def test_column_density_is_the_sky_integral(eng, lines):
    """N equals 4 pi render_field_sky(n_l) on rays from one origin: both sum
    n ds over the same crossings, the sky call as (n / (4 pi)) * ds: the
    quotient, the products and the last product one rounding each, the sums
    one per crossing a side: (2 crossings + 4) EPS"""
    o = lines["o"][5]
    d = np.concatenate([lines["d"], -lines["d"]])
    inf = np.full(len(d), np.inf)
    _, N = gpu(eng, lines, 1, -1., 1., o=o, d=d, L=inf)
    sky = eng.render_field_sky(lines["n"], o, d)
    want = 4. * np.pi * sky.T
    ratio = np.abs(N - want) / ((2 * MAX_CELLS + 4) * EPS * want)
    print("N / sky integral: %.3f of the bound" % ratio.max())
    assert (want > 0.).all() and ratio.max() <= 1.


def test_transmission_is_the_absorbing_sky_cube(eng, lines):
    """g == 0: exp(-tau) equals render_field_absorbing_sky_cube(a = S n, sl =
    0, b, background = 1) on rays from one origin. f_c is the same bits on
    both sides (the same cube_E on the same arguments). The cube forms T =
    prod (1 + expm1(-((a / dv) f ds))): per crossing the device's expm1
    (EXPM1_ULPS = 2 ulps, 4 EPS), the product and the sum (2 EPS) and four
    roundings of the argument (S n, a / dv, * f, * ds: 4 EPS tau_i), relative
    to T; tau here has four roundings per term and one per sum, (crossings +
    4) EPS tau, and numpy's exp one more. T tau <= 1 / e and T <= 1, so that
      |T - exp(-tau)| <= (6 crossings + (crossings + 8) / e + 1) EPS."""
    o = lines["o"][5]
    d = np.concatenate([lines["d"], -lines["d"]])
    inf = np.full(len(d), np.inf)
    nc, vmin, vmax = AB.axis_of(65)
    zero = np.zeros(3)
    tau, _ = gpu(eng, lines, nc, vmin, vmax, o=o, d=d, L=inf, g=zero)
    bound = (6 * MAX_CELLS + (MAX_CELLS + 8) / np.e + 1.) * EPS
    worst = 0.
    for l in range(3):
        cube = eng.render_field_absorbing_sky_cube(
            S[l] * lines["n"][l], np.zeros(BOX.n), lines["b"][l], o, d, nc,
            vmin, vmax, velocity=lines["velocity"], background=1.)
        worst = max(worst, np.abs(cube.T - np.exp(-tau[:, l])).max())
        assert cube.min() < 0.5
    print("|T - exp(-tau)| / bound = %.3f" % (worst / bound))
    assert worst <= bound


def test_cut_is_additive(eng, lines):
    """o .. o + s d and o + s d .. o + L d sum to o .. o + L d. The second
    origin is rounded, so its walk's positions, hence its path lengths, are
    off by a few EPS of the coordinates' size R over the smallest direction
    component (each wall distance is (wall - pos) / d): delta = 16 EPS R /
    min |d_a|, which moves a crossing's term by at most delta times the
    largest n S (1 / dv + wing) of the line. On top of that the sums round:
    a rounding per crossing and three per term on either side, (2 crossings +
    6) EPS tau."""
    nc, vmin, vmax = AB.axis_of(65)
    o, d = lines["o"][[5, 11, 10]], lines["d"][[5, 11, 10]]
    L = np.array([1.5, 1.5, 3.])
    s = np.array([0.9, 0.77, 1.6])
    whole = gpu(eng, lines, nc, vmin, vmax, o=o, d=d, L=L)
    first = gpu(eng, lines, nc, vmin, vmax, o=o, d=d, L=s)
    second = gpu(eng, lines, nc, vmin, vmax, o=o + s[:, None] * d, d=d,
                 L=L - s)
    R = np.abs(np.concatenate([BOX.anchor, BOX.anchor + BOX.sides])).max() + 3.
    dmin = np.abs(d[d != 0.]).min()
    delta = 16. * EPS * R / dmin
    per_length = lines["n"].max(axis=1) * S / DV + \
        AB.wing_depth(lines["n"], lines["b"], S, G)
    bound = (2 * MAX_CELLS * delta * per_length[None, :, None] +
             (2 * MAX_CELLS + 6) * EPS * whole[0])
    ratio = np.abs(first[0] + second[0] - whole[0]) / bound
    print("additivity: %.3f of the bound" % ratio.max())
    assert (first[1] > 0.).all() and (second[1] > 0.).all()
    assert ratio.max() <= 1.
    bound_N = 2 * MAX_CELLS * (delta * lines["n"].max(axis=1)[None, :] +
                               EPS * whole[1])
    assert (np.abs(first[1] + second[1] - whole[1]) <= bound_N).all()


@pytest.mark.parametrize("nchan", AB.NCHANS)
def test_parity_with_the_restatement(reference, lines, nchan):
    """every ray, line and channel within absorption_lib's bound; N exactly"""
    tau, N, rtau, rN, longest = reference[nchan]
    assert longest <= MAX_CELLS
    AD = AB.line_depth(BOX, lines["n"], S, DV)
    bound = AB.parity_bound(longest, AD, rtau)
    ratio = np.abs(tau - rtau) / np.where(bound > 0., bound, 1.)
    print("nchan %d: |gpu - cpu| / bound = %.4f" % (nchan, ratio.max()))
    assert ratio.max() <= 1.
    assert np.array_equal(N, rN)
    assert (N[[7, 8, 9]] == 0.).all() and (N[[0, 3, 4, 6]] > 0.).all()


# ----------------------------------------------------------------- physics --

def test_slab_against_the_formula(eng):
    """a uniform slab one cell thick, a ray along +x: tau_c is the contract's
    formula in numpy (math.erf against the device's: the bound of
    absorption_lib for one crossing), and far in the wing N S g / (pi (v -
    u)^2) to the accuracy Q has there: for x^2 >= 400, z = (x^2 - 0.855) /
    (x^2 + 3.42) lies in [0.9894, 1), where the polynomial 0.1117 z + 4.421
    z^2 - 9.207 z^3 + 5.674 z^4 rises from 0.9582 to its value 0.9997 at z =
    1; (1 + 21 / x^2) lies within [1, 1.0525] and x^2 / (x^2 + 1) within
    [0.9975, 1]: Q pi x^2 / a within [0.9975 * 0.9582, 1.0525 * 0.9997] =
    [0.955, 1.053], the Gaussian core being exactly 0 beyond 6 b."""
    nchan, vmin, vmax = 300, -600., 600.
    dv = (vmax - vmin) / nchan
    n0, b0, u0 = 4e9, 9., 13.
    S0, g0 = 2e-6, 0.45
    n = np.zeros(tuple(BOX.ncell))
    n[4] = n0
    b = np.full(BOX.n, b0)
    vel = np.zeros((3, BOX.n))
    vel[0] = u0
    mid = BOX.anchor + BOX.cellside * np.array([5.5, 4.5, 3.5])
    o = np.array([BOX.anchor[0] - 1., mid[1], mid[2]])
    worst = 0.
    for g in (0., g0):
        tau, N = eng.render_field_absorption_spectra(
            n.reshape(1, -1), b[None], [S0], [g], o, [(1., 0., 0.)], nchan,
            vmin, vmax, velocity=vel)
        ds = BOX.cellside[0]
        assert N[0, 0] == n0 * ds
        want = AB.crossing_tau(n0, ds, S0, g, b0, u0, nchan, vmin, vmax)
        bound = AB.parity_bound(1, [n0 * ds * S0 / dv], want[None])[0]
        worst = max(worst, (np.abs(tau[0, 0] - want) / bound).max())
        assert tau[0, 0].max() > 1.
    print("slab: |gpu - numpy| / bound = %.3f" % worst)
    assert worst <= 1.
    centres = 0.5 * (vmin + np.arange(nchan) * dv + vmin +
                     np.arange(1, nchan + 1) * dv)
    far = np.abs(centres - u0) >= 20. * b0 + dv
    lorentz = N[0, 0] * S0 * g0 / (np.pi * (centres - u0) ** 2)
    q = tau[0, 0][far] / lorentz[far]
    assert far.sum() > 100 and q.min() >= 0.955 and q.max() <= 1.053


def test_hydrogen_line_has_the_lyman_alpha_voigt_parameter():
    """the table's H I 1215.67 line: a = g / b equals the Lyman-alpha
    record's a = A21 lambda0 / (4 pi b) (csrc/lyman_alpha_kernels.h), two
    roundings apart at most (no device)"""
    from cmacionize_amd import engine as E
    ion, w, S_HI, g_HI, lam = E.absorption_table_lines(["HI_1215"])
    assert ion[0] == 0 and lam[0] == 1215.67e-10 == E.LYA_LAMBDA0
    for T in (50., 8000., 2e4):
        b = np.sqrt(2. * (1.38064852e-23 * T / (1.00794 * 1.660539040e-27)))
        a_lya = 6.265e8 * 1215.67e-10 / (4. * np.pi * b)
        assert abs(g_HI[0] / b - a_lya) <= 4. * EPS * a_lya
    # f = 0.4164 is what the Lyman-alpha mode's line-centre cross section
    # integrates to: 3 lambda0^3 A21 / (8 pi), within the literals' figures
    assert abs(S_HI[0] / (3. * lam[0] ** 3 * 6.265e8 / (8. * np.pi)) - 1.) \
        < 2e-3


def test_engine_cells_build_the_lines(eng, lines):
    """render_absorption_spectra builds n = n_H A x_ion and b = sqrt(2 k T /
    (w m_u) + 2 sigma_turb^2) on the device: it equals the field call on the
    same numbers formed in numpy but for sqrt's and the products' roundings
    (b is within 3 EPS, n within 2 EPS; compared here through N, which is
    linear in n, and through the g == 0 sum rule's S N)"""
    rng = np.random.default_rng(5)
    nH = 10. ** rng.uniform(6., 9., BOX.n)
    T = rng.uniform(5e3, 1.5e4, BOX.n)
    x = rng.uniform(0.01, 0.9, (14, BOX.n))
    eng.upload_cells(nH, T, x)
    eng.set_abundances([0.1, 2.2e-4, 4e-5, 3.3e-4, 5e-5, 9e-6])
    ions = [(0, 1.00794, S[0], 0.), (8, 15.9994, S[1], G[1])]
    o, d, ln = lines["o"], lines["d"], lines["L"]
    nc, vmin, vmax = 64, -64e3, 64e3
    tau, N = eng.render_absorption_spectra(ions, o, d, nc, vmin, vmax,
                                           lengths=ln, sigma_turb=2e3)
    n = np.array([nH * x[0], nH * 3.3e-4 * x[8]])
    b = np.sqrt(2. * 1.38064852e-23 * T[None, :] /
                (np.array([1.00794, 15.9994])[:, None] * 1.660539040e-27) +
                2. * 2e3 * 2e3)
    ftau, fN = eng.render_field_absorption_spectra(
        n, b, [S[0], S[1]], [0., G[1]], o, d, nc, vmin, vmax, lengths=ln)
    assert (fN[[0, 3, 4]] > 0.).all()
    assert (np.abs(N - fN) <= (2 + 2) * EPS * fN).all()
    # tau through b (sqrt and three operations: 3 EPS of b) and n (2 EPS): an
    # edge's E moves by |dE / dz| |z| 3 EPS <= 1.5 EPS, and two evaluations
    # of the device's erf at neighbouring arguments are each within U_DEV
    # ulps, 2 EPS each, of the truth: f moves by at most (3 + 8 U_DEV) EPS
    # absolutely; the wing is Q(g / b, x^2) / b, of order b^-2 with x^2's
    # own b^-2 inside (12 EPS), n's 2 EPS and six roundings of the term make
    # a relative 20 EPS, and the sums add 2 EPS of tau per crossing
    dv = (vmax - vmin) / nc
    AD = AB.line_depth(BOX, n, [S[0], S[1]], dv)[None, :, None]
    bound = (MAX_CELLS * (AD * (3. + 8. * AB.A.U_DEV) + 2. * ftau) +
             20. * ftau) * EPS
    assert (np.abs(tau - ftau) <= bound).all()
    assert tau.max() > 0.


# ---------------------------------------------------------------- refusals --

def test_refusals(eng, lines):
    """each refusal returns the code and leaves the outputs untouched"""
    import ctypes as C
    lib, h = eng._lib, eng._h
    _p = AB._p
    n, b = np.array(lines["n"]), np.array(lines["b"])
    vel = np.array(lines["velocity"])
    o, d, ln = (np.array(lines[k]) for k in ("o", "d", "L"))
    nc, vmin, vmax = AB.axis_of(65)

    def call(K=3, n=n, b=b, S=S, g=G, vel=vel, nrays=12, o=o, d=d, ln=ln,
             nchan=nc, vmin=vmin, vmax=vmax, null=()):
        tau = np.full((12, 3, max(nchan, 1)), -7.)
        N = np.full((12, 3), -7.)
        args = dict(n=n, b=b, S=np.array(S, dtype=float),
                    g=np.array(g, dtype=float), vel=vel, o=o, d=d, ln=ln,
                    tau=tau, N=N)
        keep = {k: np.ascontiguousarray(v) for k, v in args.items()}
        ptr = {k: (None if k in null else _p(keep[k])) for k in keep}
        rc = lib.cmi_gpu_render_field_absorption_spectra(
            h, K, ptr["n"], ptr["b"], ptr["S"], ptr["g"], ptr["vel"], nrays,
            ptr["o"], ptr["d"], ptr["ln"], None, nchan, vmin, vmax,
            ptr["tau"], ptr["N"])
        assert (tau == -7.).all() and (N == -7.).all() or rc == 0
        return rc

    def changed(x, at, value):
        y = np.array(x, dtype=float)
        y[at] = value
        return y

    assert call() == 0
    assert call(K=0) == EINVAL and call(K=17) == EINVAL
    assert call(nchan=0) == EINVAL
    assert call(vmax=vmin) == EINVAL and call(vmax=vmin - 1.) == EINVAL
    assert call(nrays=0) == 0          # an empty result, outputs untouched
    assert call(nrays=0, nchan=0) == EINVAL
    assert call(d=changed(d, (3, 0), np.nan)) == EINVAL
    assert call(d=changed(d, (3, 0), np.inf)) == EINVAL
    assert call(d=1.001 * d) == EINVAL
    assert call(o=changed(o, (2, 1), np.inf)) == EINVAL
    for bad in (0., -1., np.nan):
        assert call(ln=changed(ln, 4, bad)) == EINVAL
    for bad in (-1., np.nan, np.inf):
        assert call(n=changed(n, (1, 17), bad)) == EINVAL
        assert call(b=changed(b, (2, 5), bad)) == EINVAL
        assert call(S=changed(S, 1, bad)) == EINVAL
        assert call(g=changed(G, 0, bad)) == EINVAL
    assert call(vel=changed(vel, (0, 3), np.nan)) == EINVAL
    # absorbers of width 0 in a damped line; fine where there are none
    cell = int(np.flatnonzero(n[1] > 0.)[0])
    assert call(b=changed(b, (1, cell), 0.)) == EINVAL
    assert "width 0" in lib.cmi_gpu_last_error().decode()
    empty = int(np.flatnonzero(n[1] == 0.)[0])
    assert call(b=changed(b, (1, empty), 0.)) == 0
    for name in ("n", "b", "S", "g", "o", "d", "ln", "tau", "N"):
        assert call(null=(name,)) == EINVAL, name
    assert call(null=("vel",)) == 0
    # the engine's own ions
    ip = C.POINTER(C.c_int32)
    w = np.array([1.00794, 15.9994])
    tau = np.full((12, 2, nc), -7.)
    N = np.full((12, 2), -7.)

    def ion_call(ions, weights=w, sigma=0., engine=h):
        ions = np.array(ions, dtype=np.int32)
        return lib.cmi_gpu_render_absorption_spectra(
            engine, 2, ions.ctypes.data_as(ip), _p(weights), _p(S), _p(G),
            sigma, 12, _p(o), _p(d), _p(ln), None, nc, vmin, vmax, _p(tau),
            _p(N))

    assert ion_call([0, 14]) == EINVAL and ion_call([-1, 3]) == EINVAL
    assert ion_call([0, 8], weights=np.array([1., 0.])) == EINVAL
    assert ion_call([0, 8], sigma=-1.) == EINVAL
    assert (tau == -7.).all() and (N == -7.).all()
    from cmacionize_amd import GpuEngine
    fresh = GpuEngine(tuple(int(k) for k in BOX.ncell), tuple(BOX.anchor),
                      tuple(BOX.sides), (0, 0, 0), device=0)
    try:
        assert ion_call([0, 8], engine=fresh._h) == ESTATE
    finally:
        fresh.close()
    assert (tau == -7.).all() and (N == -7.).all()
    with pytest.raises(Exception, match="error %d" % EINVAL):
        eng.absorption_probe(n[0], b[0], S[0], G[0], o[0], d[0], MAX_CELLS,
                             nc, vmin, vmax, channels=[nc])
    with pytest.raises(Exception, match="error %d" % EINVAL):
        eng.absorption_probe(n[0], b[0], S[0], G[0], o[0], d[0], MAX_CELLS,
                             nc, vmin, vmax, channels=list(range(9)))


# ------------------------------------------------------------------- probe --

def test_probe(eng, lines, reference):
    """the probe's end value is the render call's, bit for bit; its rows are
    the restatement's cells and path lengths exactly and its running tau
    stays within the bound of its step count; with a finite length the last
    path length is the cut one"""
    nchan = 300
    nc, vmin, vmax = AB.axis_of(nchan)
    tau = reference[nchan][0]
    AD = AB.line_depth(BOX, lines["n"], S, DV)
    worst = 0.
    for r in range(12):
        for l in range(3):
            peak = int(np.argmax(tau[r, l]))
            ch = sorted({0, 63, 64, 127, 128, 255, 299, peak})
            args = (lines["n"][l], lines["b"][l], S[l], G[l], lines["o"][r],
                    lines["d"][r], MAX_CELLS, nc, vmin, vmax)
            kw = dict(channels=ch, length=lines["L"][r],
                      velocity=lines["velocity"])
            t0, t1, steps, cells, ds, run, end = AB.split_probe(
                eng.absorption_probe(*args, **kw), MAX_CELLS, len(ch))
            c0, c1, csteps, ccells, cds, crun, cend = AB.split_probe(
                AB.probe(BOX, *args, **kw), MAX_CELLS, len(ch))
            assert np.array_equal(end, tau[r, l][ch]), (r, l)
            assert steps == csteps and np.array_equal(cells, ccells)
            assert np.array_equal(ds, cds)
            assert np.array_equal([t0, t1], [c0, c1], equal_nan=True)
            for i in range(steps):
                bound = AB.parity_bound(i + 1, AD[l:l + 1], crun[None, :, i])
                ok = bound[0] > 0.
                assert np.array_equal(run[~ok, i], crun[~ok, i])
                if ok.any():
                    worst = max(worst, (np.abs(run[ok, i] - crun[ok, i]) /
                                        bound[0][ok]).max())
            if steps:
                assert np.array_equal(run[:, steps - 1], end)
            if np.isfinite(lines["L"][r]) and steps and lines["L"][r] < t1:
                # the running sum of the path lengths, as the contract forms it
                t = t0
                for i in range(steps - 1):
                    t = t + ds[i]
                assert ds[steps - 1] == lines["L"][r] - t
    print("probe: running |gpu - cpu| / bound = %.4f" % worst)
    assert worst <= 1.
